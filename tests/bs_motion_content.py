"""Motion that reaches every branch of derive_boundaryStrength, and a census of what it decided (tests/test_bs_motion.py).

The generator draws every vector uniformly from +-64 quarter samples (csrc/synth.c gen_pb), so two neighbouring prediction blocks
almost never name the same pictures with vectors less than 4 apart: on its pictures the motion part of the boundary strength
(deblock.cc:294-361) returns 1 for nearly every edge between two PBs; the threshold itself, the crossed comparison, the conjunction
for two lists on one picture and the outcome 0 are reached by chance, if at all.

motion_field() keeps the generator's block structure and rewrites the motion.  The coding units form a checkerboard: the `A` units of a
region carry the region's base motion, each `B` unit the base plus ONE deciding difference `delta` (in x or y, of either sign, on the
first or second vector pair: its variant) and differences of at most 3 everywhere else, so an edge between two units is decided by that
one comparison, and P - Q has either sign (P is A at one edge and B at the next).  The regions of the plan hold the cases of the function:
  ONE_STRAIGHT  one list each, the same list (L0 or L1)   ONE_CROSS  one list each, L0 against L1, one picture
  TWO_STRAIGHT  two pictures, the same order              TWO_CROSS  two pictures, the lists swapped
  TWO_SAME      both lists name one picture on both sides: the conjunction of the straight and the crossed comparison — B units that
                hang one conjunct on delta while the other is far (1 with delta 4, 0 with 3), that keep one near and one far (0), and, in
                every second pair of unit columns, units whose four vectors are all within 3 of each other (0)
  FILL          both references missing (PBF_FILL_*, slot n_refs)
TWINS are the same picture with delta = 3 and delta = 4: what is bS 0 in one is bS 1 in the other.  The unused list of a
uni-predicted block holds a stale slot and vector that differ between neighbours.  With `wrap`, the first two units of every region
at least three units wide have x vectors of 32767 and -32766: a difference of 65533, which is -3 in 16 bits (record_checks.h has no
bound on vectors; the kernels clamp the window as the reference does).  Such blocks predict the replicated border column instead of
the ramp; the offset of the second of the pair levels the step at their common edge to S again, their other edges are what they
are — so the pair lives in a third picture beside the twins, and only its own segments are asked to be live there.
The two blocks of a two-block unit have the same motion and different offsets: bS 0 at the internal edge, which is on the 8-grid
for 2NxN / Nx2N (and the AMP modes of a 32x32 unit: 8 / 24) and off it for the AMP modes of a 16x16 unit (4 / 12).  The first two such
units with an edge on the grid and ONE transform leaf are marked coded (cbf_luma): E_NONZERO on both sides of an edge that is no TU
edge, bS 0; the first with a split tree too: the same edge is a TU edge, bS 1.  (Their outer edges become coded TU edges, hence so few.)
Every block is predicted with explicit weights (w = 1, log2WD = shift1) and an offset of its own: S = 4 << (bd - 8) in A, 0 in B,
2S / -S in their second blocks, from references that are one ramp (deblock_content.ramp_plane) in every slot — every edge between two
blocks is a step of S, 2S or 3S in smooth content, which the filter changes where bS is 1, and the step never comes from a coefficient.
Intra units (a case of its own) stay as the generator made them.

bs_reference() restates deblock.cc:132-383 on the work lists (edge flags from CUs, partition modes and transform leaves; the strength
from the blocks on both sides) and names, for every 4-sample segment of the 8-grid, the class and which comparison decided.  It is
checked against the oracle through the planes: bs_census() counts per class the segments that are LIVE — a sample p2..q2 changed on the
segment's line that the other pass cannot write (as deblock_content._one_sided judges) — and a segment with bS 0 must be silent.
The census of the seeds in use is in the header of tests/test_bs_motion.py."""
import numpy as np

from deblock_content import ramp_plane
from libde265_amd import synth, worklist as W

NO_EDGE, INTRA, CODED_TU_EDGE, SAME_PB, REFS_DIFFER, ONE_STRAIGHT, ONE_CROSS, TWO_STRAIGHT, TWO_CROSS, TWO_SAME, FILL = range(11)
NAMES = ["NO_EDGE", "INTRA", "CODED_TU_EDGE", "SAME_PB", "REFS_DIFFER", "ONE_STRAIGHT", "ONE_CROSS", "TWO_STRAIGHT", "TWO_CROSS",
         "TWO_SAME", "FILL"]
COMPARED = (ONE_STRAIGHT, ONE_CROSS, TWO_STRAIGHT, TWO_CROSS, TWO_SAME, FILL)
TU_V, TU_H, PB_V, PB_H = 1, 2, 4, 8
WRAP = 16000          # a vector beyond this magnitude is one of a 65533 pair

BASE = dict(intra_pct=0, cbf_pct=0, weighted_pct=0, oob_mv_pct=0, sao=0, n_refs=2, fixed_cu_log2=4)


# ------------------------------------------------------------------------------------------------------------------ the lists as maps
class Maps:
    """per 4x4 unit: CU index, PB index (+ 1, 0 = none), slice index, tile id, cbf_luma; per CU its transform leaves"""

    def __init__(self, pic):
        pp = pic.pp[0]
        self.w, self.h = int(pp["width"]), int(pp["height"])
        self.w4, self.h4 = self.w // 4, self.h // 4
        cs = int(pp["log2_ctb_size"])
        self.cu = np.zeros((self.h4, self.w4), np.int64)
        self.pb = np.zeros((self.h4, self.w4), np.int64)
        self.nz = np.zeros((self.h4, self.w4), bool)
        for i, c in enumerate(pic.cus):
            n = (1 << int(c["log2_size"])) // 4
            self.cu[int(c["y"]) // 4:int(c["y"]) // 4 + n, int(c["x"]) // 4:int(c["x"]) // 4 + n] = i + 1
        for i, p in enumerate(pic.pbs):
            self.pb[int(p["y"]) // 4:(int(p["y"]) + int(p["h"])) // 4, int(p["x"]) // 4:(int(p["x"]) + int(p["w"])) // 4] = i + 1
        self.tus_of = {}
        for t in pic.tus:
            x, y, n = int(t["x"]), int(t["y"]), 1 << int(t["log2_size"])
            if int(t["flags"]) & W.TUF_NONZERO_COEFF:
                self.nz[y // 4:(y + n) // 4, x // 4:(x + n) // 4] = True
            self.tus_of.setdefault(int(self.cu[y // 4, x // 4]), []).append((x, y, n))
        ctbw = (self.w + (1 << cs) - 1) >> cs
        ncols, nrows = int(pp["num_tile_cols"]), int(pp["num_tile_rows"])
        col_bd, row_bd = [int(v) for v in pp["col_bd"][:ncols + 1]], [int(v) for v in pp["row_bd"][:nrows + 1]]
        self.slice = np.zeros((self.h4, self.w4), np.int64)
        self.tile = np.zeros((self.h4, self.w4), np.int64)
        for y4 in range(self.h4):
            cy = (y4 * 4) >> cs
            ty = max(k for k in range(nrows) if row_bd[k] <= cy)
            for x4 in range(self.w4):
                cx = (x4 * 4) >> cs
                self.slice[y4, x4] = int(pic.ctbs[cy * ctbw + cx]["slice_idx"])
                self.tile[y4, x4] = ty * ncols + max(k for k in range(ncols) if col_bd[k] <= cx)


def edge_flags(pic, m):
    """derive_edgeFlags (deblock.cc:132-240) with markTransformBlockBoundary on the leaves and markPredictionBlockBoundary"""
    pp = pic.pp[0]
    ctb_mask = (1 << int(pp["log2_ctb_size"])) - 1
    across_tiles = bool(int(pp["flags"]) & W.PF_LF_ACROSS_TILES)
    ef = np.zeros((m.h4, m.w4), np.int64)
    for i, c in enumerate(pic.cus):
        x0, y0, cb = int(c["x"]), int(c["y"]), 1 << int(c["log2_size"])
        sh = pic.slices[m.slice[y0 // 4, x0 // 4]]
        across = bool(int(sh["flags"]) & W.SF_LF_ACROSS_SLICES)
        left, top = x0 != 0, y0 != 0
        if x0 and (x0 & ctb_mask) == 0:
            other = pic.slices[m.slice[y0 // 4, (x0 - 1) // 4]]
            if not across and int(other["slice_addr_rs"]) != int(sh["slice_addr_rs"]):
                left = False
            elif not across_tiles and m.tile[y0 // 4, x0 // 4] != m.tile[y0 // 4, (x0 - 1) // 4]:
                left = False
        if y0 and (y0 & ctb_mask) == 0:
            other = pic.slices[m.slice[(y0 - 1) // 4, x0 // 4]]
            if not across and int(other["slice_addr_rs"]) != int(sh["slice_addr_rs"]):
                top = False
            elif not across_tiles and m.tile[y0 // 4, x0 // 4] != m.tile[(y0 - 1) // 4, x0 // 4]:
                top = False
        if int(sh["flags"]) & W.SF_DEBLOCK_DISABLED:
            continue
        for (x, y, n) in m.tus_of.get(i + 1, []):
            if x != x0 or left:
                ef[y // 4:(y + n) // 4, x // 4] |= TU_V
            if y != y0 or top:
                ef[y // 4, x // 4:(x + n) // 4] |= TU_H
        pm = int(c["part_mode"])
        vx = {3: cb // 2, 2: cb // 2, 6: cb // 4, 7: cb // 2 + cb // 4}.get(pm)
        hy = {3: cb // 2, 1: cb // 2, 4: cb // 4, 5: cb // 2 + cb // 4}.get(pm)
        if vx is not None:
            ef[y0 // 4:(y0 + cb) // 4, (x0 + vx) // 4] |= PB_V
        if hy is not None:
            ef[(y0 + hy) // 4, x0 // 4:(x0 + cb) // 4] |= PB_H
    return ef


def _motion(pb):
    """(refPic0, refPic1, mv0, mv1, all used lists are fills) of a block, as deblock.cc:302-317 reads them (RefPicList[l][k] = slot k)"""
    f = int(pb["flags"])
    use = [bool(f & W.PBF_PRED_L0), bool(f & W.PBF_PRED_L1)]
    r = [int(pb["ref_slot"][k]) if use[k] else -1 for k in (0, 1)]
    mv = [(int(pb["mv"][k][0]), int(pb["mv"][k][1])) if use[k] else (0, 0) for k in (0, 1)]
    fill = all(bool(f & (W.PBF_FILL_L0 << k)) for k in (0, 1) if use[k])
    return r[0], r[1], mv[0], mv[1], fill


def _tests(pairs):
    """the component tests of one `||` chain of deblock.cc:331-358 -> list of (pair, component, P - Q)"""
    return [(k, c, a[c] - b[c]) for k, (a, b) in enumerate(pairs) for c in (0, 1)]


def _compare(P, Q):
    """the motion part (deblock.cc:302-361) -> (bS, class, info); info: outcome, decider = (component, sign, pair) where ONE test alone
    made the outcome 1 (outcome 0: the largest difference, where it is unique), mag = that difference, conj (TWO_SAME: which conjunct is far)"""
    rP0, rP1, p0, p1, fP = P
    rQ0, rQ1, q0, q1, fQ = Q
    if not ((rP0 == rQ0 and rP1 == rQ1) or (rP0 == rQ1 and rP1 == rQ0)):
        return 1, REFS_DIFFER, None
    straight, cross = _tests([(p0, q0), (p1, q1)]), _tests([(p0, q1), (p1, q0)])
    conj = None
    if rP0 != rP1:
        two = rP0 >= 0 and rP1 >= 0
        if rP0 == rQ0:
            chain, cls = straight, TWO_STRAIGHT if two else ONE_STRAIGHT
        else:
            chain, cls = cross, TWO_CROSS if two else ONE_CROSS
        bs = int(any(abs(d) >= 4 for _, _, d in chain))
    else:
        cls = TWO_SAME
        far = [any(abs(d) >= 4 for _, _, d in ch) for ch in (straight, cross)]
        conj = tuple(far)
        bs = int(far[0] and far[1])
        # the conjunct that the outcome hangs on: the one with fewer far tests
        chain = min((straight, cross), key=lambda ch: sum(abs(d) >= 4 for _, _, d in ch))
    cls16 = cls
    if fP and fQ:
        cls = FILL
    far_tests = [t for t in chain if abs(t[2]) >= 4]
    if bs:
        sole = far_tests[0] if len(far_tests) == 1 else None
    else:
        top = max(abs(d) for _, _, d in chain)
        best = [t for t in chain if abs(t[2]) == top]
        sole = best[0] if len(best) == 1 and not far_tests else None
    # what the same comparison gives with the differences taken in 16 bits
    s16 = [[abs((d + 32768) % 65536 - 32768) >= 4 for _, _, d in ch] for ch in (straight, cross)]
    short = int(any(s16[0]) and any(s16[1])) if cls16 == TWO_SAME else int(any(s16[0] if chain is straight else s16[1]))
    info = dict(outcome=bs, short=short, conj=conj, decider=None if sole is None else (sole[1], 1 if sole[2] > 0 else -1, sole[0]),
                mag=None if sole is None else abs(sole[2]))
    return bs, cls, info


def bs_reference(pic):
    """-> list of dict(vertical, x, y, bs, cls, info, wrap) for every 4-sample segment of the 8-grid, both directions; (x, y) is the
    segment's first Q sample.  wrap: a block on either side holds a vector of a 65533 pair."""
    m = Maps(pic)
    ef = edge_flags(pic, m)
    mot = [_motion(p) for p in pic.pbs]
    big = [any(abs(v) > WRAP for k in (0, 1) if mo[k] >= 0 for v in mo[2 + k]) for mo in mot]
    out = []
    for vertical in (True, False):
        em, tm = (TU_V | PB_V, TU_V) if vertical else (TU_H | PB_H, TU_H)
        for y4 in range(0, m.h4, 1 if vertical else 2):
            for x4 in range(0, m.w4, 2 if vertical else 1):
                if (x4 if vertical else y4) == 0:
                    continue                                   # the picture's border: not a segment
                xo, yo = (x4 - 1, y4) if vertical else (x4, y4 - 1)
                e = int(ef[y4, x4])
                info, wrap = None, False
                cup, cuq = pic.cus[m.cu[yo, xo] - 1], pic.cus[m.cu[y4, x4] - 1]
                if not (e & em):
                    bs, cls = 0, NO_EDGE
                elif int(cup["pred_mode"]) == 0 or int(cuq["pred_mode"]) == 0:
                    bs, cls = 2, INTRA
                elif (e & tm) and (m.nz[y4, x4] or m.nz[yo, xo]):
                    bs, cls = 1, CODED_TU_EDGE
                else:
                    ip, iq = int(m.pb[yo, xo]), int(m.pb[y4, x4])
                    assert ip and iq, "an inter unit without a prediction block"
                    bs, cls, info = _compare(mot[ip - 1], mot[iq - 1])
                    wrap = big[ip - 1] or big[iq - 1]
                    if ip == iq:
                        assert bs == 0
                        cls, info = SAME_PB, None
                out.append(dict(vertical=vertical, x=4 * x4, y=4 * y4, bs=bs, cls=cls, info=info, wrap=wrap,
                                internal=m.cu[yo, xo] == m.cu[y4, x4], nz=bool(m.nz[y4, x4] and m.nz[yo, xo]),
                                inter_side=int(cup["pred_mode"]) != 0 or int(cuq["pred_mode"]) != 0,
                                pcm_side=bool((int(cup["flags"]) | int(cuq["flags"])) & W.CUF_PCM)))
    return out


# ---------------------------------------------------------------------------------------------------------------------- the content
def default_plan(width, height, cu):
    """(x0, y0, x1, y1, class): FILL in a strip two units wide on the left; beside it three bands of a third of the height each:
    ONE_STRAIGHT | TWO_CROSS, TWO_SAME over the whole width (it has the most placements), ONE_CROSS | TWO_STRAIGHT"""
    ys = [(k * height // 3) // cu * cu for k in range(3)] + [height]
    x0 = 2 * cu
    xm = (x0 + width) // 2 // cu * cu
    return [(0, 0, x0, height, FILL),
            (x0, ys[0], xm, ys[1], ONE_STRAIGHT), (xm, ys[0], width, ys[1], TWO_CROSS),
            (x0, ys[1], width, ys[2], TWO_SAME),
            (x0, ys[2], xm, ys[3], ONE_CROSS), (xm, ys[2], width, ys[3], TWO_STRAIGHT)]


def band_plan(width, height, cu):
    """every class in a band over the whole width, so that a tile column has both its sides in every class; two unit rows for TWO_SAME
    and TWO_CROSS, one for the others (these have no horizontal edge of their own) — for a picture eight units high"""
    rows = [(TWO_SAME, 2), (ONE_STRAIGHT, 1), (ONE_CROSS, 1), (TWO_CROSS, 2), (TWO_STRAIGHT, 1), (FILL, 1)]
    assert height == cu * sum(n for _, n in rows)
    plan, y = [], 0
    for cls, n in rows:
        plan.append((0, y, width, y + n * cu, cls))
        y += n * cu
    return plan


A0, A1 = (9, -6), (-14, 11)          # a region's base vectors: more than 4 apart from each other in both components
N0, N1 = (2, -3), (-3, 1)            # differences that stay below the threshold
L0, L1 = W.PBF_PRED_L0 | W.PBF_MC_L0, W.PBF_PRED_L1 | W.PBF_MC_L1


def _add(a, b):
    return (a[0] + b[0], a[1] + b[1])


def _unit_motion(cls, b_unit, rx, ry, rw, delta, n_refs, k, seed):
    """(flags, slots, mv0, mv1) of the unit at unit position (rx, ry) of region k (class cls, rw units wide).  An A unit (b_unit
    False) holds the region's base motion; the j-th B unit of the region the base plus `delta` on the component / pair that j selects
    (its sign changes with j too; P - Q has both signs anyway), and differences below the threshold on everything else.  `alt` is a
    second flavour, for A and B alike: in every second pair of unit columns (and rows) ONE_STRAIGHT / FILL use L1 instead of L0 and ONE_CROSS
    swaps which of A and B uses L0; in the last two unit columns of TWO_SAME all four vectors of both sides lie within delta"""
    j = (ry * rw + rx) // 2 + seed                              # (the B units of a row are every second unit)
    comp, pair, sgn = j & 1, (j >> 1) & 1, 1 if j & 4 else -1
    d = (sgn * delta, N0[1]) if comp == 0 else (N0[0], sgn * delta)
    a0, a1 = _add(A0, (k, -k)), _add(A1, (-k, k))
    if cls in (ONE_STRAIGHT, FILL, ONE_CROSS):
        alt = ((rx >> 1) ^ (ry >> 1)) & 1
        mine = alt if cls != ONE_CROSS else (alt ^ int(b_unit))
        flags = (L1 if mine else L0) | ((W.PBF_FILL_L0 << mine) if cls == FILL else 0)
        # the list that is not used holds a stale slot and vector, other ones in A than in B
        slots = [1, 1] if b_unit else [0, 0]
        mvs = [_add((40, -40), (j & 7, k))] * 2 if b_unit else [_add((-23, 31), (k, j & 7))] * 2
        slots[mine], mvs[mine] = (n_refs if cls == FILL else k % n_refs), (_add(a0, d) if b_unit else a0)
        return flags, slots, mvs[0], mvs[1]
    if cls in (TWO_STRAIGHT, TWO_CROSS):
        if not b_unit:
            return L0 | L1, [0, 1], a0, a1
        b = [_add(a0, d), _add(a1, N1)] if pair == 0 else [_add(a0, N1), _add(a1, d)]
        return (L0 | L1, [0, 1], b[0], b[1]) if cls == TWO_STRAIGHT else (L0 | L1, [1, 0], b[1], b[0])
    assert cls == TWO_SAME
    slot = k % n_refs
    if rx >= rw - 2:                       # both conjuncts hang on delta: near and near (0) with 3, far and far (1) with 4
        a1 = a0
        b = [_add(a0, (sgn * delta, 0) if comp == 0 else (0, sgn * delta)), a0]
    else:
        sel = (ry * ((rw - 2) // 2) + rx // 2 + seed) & 3          # (the B units outside the last two columns, in order)
        if sel == 0:                       # the straight conjunct hangs on delta (x, first pair), the crossed one is far
            b = [_add(a0, (sgn * delta, N0[1])), _add(a1, N1)]
        elif sel == 2:                     # the crossed conjunct hangs on delta (y, second pair: P's second vector against Q's first)
            b = [_add(a1, (N0[0], sgn * delta)), _add(a0, N1)]
        elif sel == 1:                     # straight far, crossed near: 0 whatever delta is
            b = [_add(a1, N1), _add(a0, N0)]
        else:                              # straight near, crossed far: 0
            b = [_add(a0, N0), _add(a1, N1)]
    return (L0 | L1, [slot, slot], b[0], b[1]) if b_unit else (L0 | L1, [slot, slot], a0, a1)


def _internal_on_grid(cu):
    """the unit has two blocks and the edge between them lies on the 8-grid"""
    pm, n = int(cu["part_mode"]), 1 << int(cu["log2_size"])
    return pm in (1, 2) or (pm >= 4 and n >= 32)


def motion_field(pic, plan, delta, seed, wrap=True, coded=True):
    """A copy of `pic` with the motion, the weights and the cbf marks of the module's header -> (picture, references).
    plan: list of (x0, y0, x1, y1, class); delta: the deciding difference; seed: shifts which unit gets which variant."""
    out = pic.copy()
    pp = out.pp[0]
    bd, bdc, n_refs = int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"]), int(pic.meta["cfg"]["n_refs"])
    m = Maps(out)
    S, Sc = 4 << (bd - 8), 4 << (bdc - 8)
    gap8 = (int(pp["width"]) - 1) >> 2                       # last column minus first column of the ramp, in 8-bit levels
    wts = np.zeros(len(out.pbs), W.WT)
    wts["w"] = 1
    wts["log2wd_luma"], wts["log2wd_chroma"] = max(2, 14 - bd), max(2, 14 - bdc)
    seen, marked = set(), [0, 0]
    for i, pb in enumerate(out.pbs):
        x, y = int(pb["x"]), int(pb["y"])
        ci = int(m.cu[y // 4, x // 4])
        cu = out.cus[ci - 1]
        n = 1 << int(cu["log2_size"])
        ux, uy = int(cu["x"]) // n, int(cu["y"]) // n
        k = [j for j, r in enumerate(plan) if r[0] <= x < r[2] and r[1] <= y < r[3]][0]
        cls = plan[k][4]
        b_unit = bool((ux + uy) & 1)
        second = ci in seen
        seen.add(ci)
        rx, ry = (int(cu["x"]) - plan[k][0]) // n, (int(cu["y"]) - plan[k][1]) // n
        flags, slots, mv0, mv1 = _unit_motion(cls, b_unit, rx, ry, (plan[k][2] - plan[k][0]) // n, delta, n_refs, k, seed & 7)
        mvs = [list(mv0), list(mv1)]
        o = (-S if second else 0) if b_unit else (2 * S if second else S)     # (a unit's second block: the same motion, another offset)
        if wrap and ry == 0 and rx < 2 and plan[k][2] - plan[k][0] >= 3 * n:
            # the 65533 pair: the region's first two units, x of the vectors that the edge between them compares
            both = (flags & W.PBF_PRED_L0) and (flags & W.PBF_PRED_L1)
            lst = (rx if cls == TWO_CROSS else 0) if both else (0 if flags & W.PBF_PRED_L0 else 1)
            mvs[lst][0] = -32766 if rx else 32767
            if rx and cls != FILL:
                # first column against last, in one list of one or two (offsets are whole 8-bit levels: slice.cc:159-231 stores them so)
                o += (gap8 // (2 if both else 1)) << (bd - 8)
        out.pbs["flags"][i] = flags | W.PBF_WEIGHTED
        out.pbs["ref_slot"][i] = slots
        out.pbs["mv"][i] = mvs
        out.pbs["wt_idx"][i] = [i, i]
        wts["o"][i] = [o, (o * Sc) // S, (o * Sc) // S]
        if coded and not second and _internal_on_grid(cu):
            # coded units: the first two whose transform tree is one leaf (the internal edge is no TU edge), the first one with a split tree
            leaves = [t for t in range(len(out.tus)) if int(m.cu[int(out.tus["y"][t]) // 4, int(out.tus["x"][t]) // 4]) == ci]
            kind = 0 if len(leaves) == 1 else 1
            if marked[kind] < (2, 1)[kind]:
                marked[kind] += 1
                out.tus["flags"][leaves] |= W.TUF_NONZERO_COEFF
    out.wts = wts
    dt = np.uint8 if bd <= 8 else np.uint16
    dims = W.plane_dims(int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]))
    refs = [[ramp_plane(ph, pw, bdc if c else bd, dt) for c, (pw, ph) in enumerate(dims) if pw] for _ in range(n_refs)]
    return out, refs


def make_bs_case(delta, plan=default_plan, wrap=True, coded=True, slice_flags=None, **cfg):
    """the generator's picture for BASE + cfg with the directed motion -> (picture, references, plan)"""
    full = dict(BASE)
    full.update(cfg)
    pic = synth.picture(**full)
    pp = pic.pp[0]
    for k, fl in enumerate(slice_flags or []):
        assert k < len(pic.slices), "the generator made fewer slices than the case names"
        pic.slices["flags"][k] = fl
        pic.slices["beta_offset"][k] = pic.slices["tc_offset"][k] = 0
    regions = plan(int(pp["width"]), int(pp["height"]), 1 << full["fixed_cu_log2"])
    pic, refs = motion_field(pic, regions, delta, full.get("seed", 1), wrap, coded)
    return pic, refs, regions


# ----------------------------------------------------------------------------------------------------------------------- the census
def segment_live(ch, seg):
    """ch: luma samples that the stage changed (bool) -> one of p2..q2 changed on the segment's line the other pass cannot write"""
    c = ch if seg["vertical"] else ch.T
    x, y = (seg["x"], seg["y"]) if seg["vertical"] else (seg["y"], seg["x"])
    line = y + 3 if (y & 7) == 0 else y
    return bool(c[line, x - 3:x + 3].any())


def bs_census(pic, pre, post, segs=None):
    """-> (segments with `live` set, counts {(class, outcome or bS, vertical): [segments, live]}); pre / post: the oracle's planes
    before and after the deblocking stage"""
    segs = bs_reference(pic) if segs is None else segs
    ch = pre[0] != post[0]
    counts = {}
    for s in segs:
        s["live"] = segment_live(ch, s)
        key = (s["cls"], s["info"]["outcome"] if s["info"] else s["bs"], s["vertical"])
        n = counts.setdefault(key, [0, 0])
        n[0] += 1
        n[1] += int(s["live"])
    return segs, counts
