"""Pictures whose QP walks the whole legal range, and a restatement of what the deblocking filter makes of them (tests/test_deblock_qp_range.py).

The generator draws QpY from 22..37, fixes the picture's chroma offsets at +1 / -1 and the slice offsets within +-4 (+-6), so the inputs of the
beta / tc tables and of the chroma QP map (deblock.cc:397-407, transform.h:29-34) stay in a window: beta entries 38..51, tc entries 40..53, both
Clip3 bounds of both indices, the zero regions below 16 / 18, the upper half of the 4:2:0 map and the min(qP_i, 51) of the other formats are
reached by a few `qp_wide` seeds or not at all.

qp_picture() keeps a generated picture's block structure (16x16 units in 32x32 CTBs, the units' partitions and transform trees) and rewrites
  cus["qp_y"]     a field  qmin + (a + sx * ux + sy * uy) mod (52 - qmin)  over the units (ux, uy), qmin = -QpBdOffsetY: with sx = 1 the averages
                  (QP_Q + QP_P + 1) >> 1 at the vertical edges of a unit row are consecutive values from odd sums, with an even sy those at the
                  horizontal edges come from even sums, with an odd sy from odd ones
  pp["pic_cb_qp_offset"], pp["pic_cr_qp_offset"]   one pair per picture, -12..12
  slices          the picture is cut into one slice per CTB row (per tile, where it has tiles), each with its own even beta / tc offsets in -12..12
and makes every sample on both sides of every edge the test's own:
  inter units     predict from list 0 with a zero vector, unweighted, from references that all hold the CANVAS: the prediction is the canvas.
                  Slots alternate like a checkerboard, so two inter units never name the same picture: bS 1 (deblock.cc:319-327)
  PCM units       every third or second unit (all of them in the all-intra and the 16-bit pictures: motion compensation keeps 14 bits and has
                  no exact copy of a 16-bit sample) becomes a PCM unit whose raw samples are the canvas: bS 2 beside
                  it, which the chroma filter needs.  pcm_loop_filter_disable stays off.
No unit carries a residual.  The canvas is flat (mid level) but for
  luma    the two middle segments of every unit edge (4 lines each; the two at the corners of a unit, which both passes touch, stay flat and
          silent), designed from the segment's own beta and tc: both sides flat with a step whose weak-filter delta is tc' + 2 table units
          (between tc and 10 tc: the filter writes p0 + tc, q0 - tc), and p2, p3 raised so that d = dp0 + dp3 is beta - 1 (the filter is on;
          one table unit less and it is off) or, in the second segment of every second edge, exactly beta (off; one unit more and it is on).
          Where tc' or beta' is 0 the step is that of tc' = 1, beta' = 6: the segment must stay silent
  chroma  every unit flat, 28 table units above or below mid level like a checkerboard: delta = +-28 > 24 at every edge, the filter writes
          p0 + tc, q0 - tc wherever tc > 0.  Cb and Cr get the same canvas, so they differ after the filter where their tc differs.
Directed segments never share a sample, so each is an experiment of its own.

restate() follows deblock.cc:480-605 and :635-761 with fallback-deblk.h:33-124 on the lists and the canvas (boundary strengths from
bs_motion_content.bs_reference): first all vertical edges, then all horizontal ones.  For every filtered segment it records the unclipped index
sums, the indices, per chroma plane qP_i, QP_C and the tc index, and which one-step changes of the tables its output is SENSITIVE to: the
segment is filtered again with that change alone and the result compared on the lines the other pass cannot write.  The changes:
  beta-, beta+  the segment's c_tab_beta entry one less / one more       tc-, tc+  the same for c_tab_tc
  beta_hi, tc_hi  the upper Clip3 bound one lower (50 / 52)              round     (QP_Q + QP_P) >> 1 without the + 1
  qpc-, qpc+    (chroma) QP_C one less / one more: what a wrong entry of the 4:2:0 table, `- 5` for `- 6`, or a wrong branch gives
  nomin         (chroma, not 4:2:0) QP_C = qP_i without the min
(The neighbouring ENTRY's value would not do as the change: c_tab_tc holds runs of equal values.)  census() counts them."""
import numpy as np

from bs_motion_content import bs_reference
from libde265_amd import synth, worklist as W

TAB_BETA = [0] * 16 + [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60,
                       62, 64]
TAB_TC = [0] * 18 + [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24]
TAB_QPC_420 = [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37]       # qP_i 30..42
assert len(TAB_BETA) == 52 and len(TAB_TC) == 54

CU = 16
BASE = dict(width=128, height=96, log2_ctb=5, fixed_cu_log2=4, intra_pct=0, cbf_pct=0, weighted_pct=0, oob_mv_pct=0, bipred_pct=0, n_refs=2)
LUMA_CHANGES = ("beta-", "beta+", "tc-", "tc+", "beta_hi", "tc_hi", "round")
CHROMA_CHANGES = ("tc-", "tc+", "tc_hi", "round", "qpc-", "qpc+", "nomin")
CHROMA_STEP = 56          # table units: delta = (4 * 56 + 4) >> 3 = 28 > 24, the largest tc'


def clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


# ----------------------------------------------------------------------------------------------------------------------- the lists
def qp_field(spec, bd, nx, ny):
    qmin = -6 * (bd - 8)
    span = 52 - qmin
    return [[qmin + (spec["a"] - qmin + spec.get("sx", 1) * ux + spec.get("sy", 8) * uy) % span for ux in range(nx)] for uy in range(ny)]


def is_pcm(spec, ux, uy):
    m = spec.get("pcm_mod", 3)
    return m == 1 or (m > 1 and (ux + 2 * uy + spec.get("pcm_phase", 0)) % m == 0)


def _cut_slices(pic, offsets):
    """one slice per CTB row, or per tile where the picture has tiles, with the offsets of the list in turn (the last slice takes the rest)"""
    pp = pic.pp[0]
    ctbw, ctbh = pic.pic_w_ctbs, pic.pic_h_ctbs
    ncols, nrows = int(pp["num_tile_cols"]), int(pp["num_tile_rows"])
    starts = []                                           # (first CTB in raster order, its CTBs)
    if ncols * nrows > 1:
        cb, rb = [int(v) for v in pp["col_bd"][:ncols + 1]], [int(v) for v in pp["row_bd"][:nrows + 1]]
        for ty in range(nrows):
            for tx in range(ncols):
                starts.append([cy * ctbw + cx for cy in range(rb[ty], rb[ty + 1]) for cx in range(cb[tx], cb[tx + 1])])
    else:
        n = min(len(offsets), ctbh)
        for k in range(n):
            last = ctbh if k == n - 1 else k + 1
            starts.append([cy * ctbw + cx for cy in range(k, last) for cx in range(ctbw)])
    sl = np.zeros(len(starts), W.SLICE)
    for k, ctbs in enumerate(starts):
        sl["slice_addr_rs"][k] = ctbs[0]
        sl["beta_offset"][k], sl["tc_offset"][k] = offsets[k % len(offsets)]
        sl["flags"][k] = W.SF_LF_ACROSS_SLICES | W.SF_SAO_LUMA | W.SF_SAO_CHROMA
        pic.ctbs["slice_idx"][ctbs] = k
    pic.slices = sl


def _pcm_blocks(x, y, cf):
    """the raw blocks of a PCM unit at (x, y): (cidx, x, y, log2) in component samples; 4:2:2 chroma is two stacked squares"""
    out = [(0, x, y, 4)]
    if cf:
        subw, subh = int(cf in (1, 2)), int(cf == 1)
        l2 = 4 - subw
        for cidx in (1, 2):
            for b in range(2 if subw and not subh else 1):
                out.append((cidx, x >> subw, (y >> subh) + b * (1 << l2), l2))
    return out


def rewrite_lists(gen, spec):
    """a copy of the generator's picture `gen` with the QP field, the offsets, the slices and the units' kinds of `spec`; PCM samples are 0 yet"""
    pic = gen.copy()
    pp = pic.pp[0]
    cf, bd = int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"])
    w, h = int(pp["width"]), int(pp["height"])
    assert w % CU == 0 and h % CU == 0 and int(pp["log2_ctb_size"]) == 5 and all(int(v) == 4 for v in pic.cus["log2_size"])
    assert len(pic.rbs) == 0 and len(pic.wts) == 0, "the generated picture carries residuals or weights"
    n_refs = int(gen.meta["cfg"]["n_refs"])
    qp = qp_field(spec, bd, w // CU, h // CU)
    pic.pp["pic_cb_qp_offset"], pic.pp["pic_cr_qp_offset"] = spec["cb"], spec["cr"]
    _cut_slices(pic, spec["slices"])
    # transform leaves of every unit, as generated
    leaves = {}
    for k, t in enumerate(gen.tus):
        leaves.setdefault((int(t["x"]) // CU, int(t["y"]) // CU), []).append(k)
    ctbw = pic.pic_w_ctbs
    cus_of = {}
    for i, c in enumerate(pic.cus):
        cus_of.setdefault((int(c["y"]) >> 5) * ctbw + (int(c["x"]) >> 5), []).append(i)
    pcm_units, tus, ibs, n_pcm = set(), [], [], 0
    order = np.argsort(pic.ctbs["ib_start"], kind="stable") if len(pic.ibs) else np.arange(len(pic.ctbs))
    pic.ctbs["flags"] &= ~np.uint8(W.CTBF_HAS_PCM_OR_BYPASS)
    for a in [int(v) for v in order]:
        pic.ctbs["ib_start"][a] = len(ibs)
        for i in cus_of.get(a, []):
            c = pic.cus[i]
            x, y = int(c["x"]), int(c["y"])
            ux, uy = x // CU, y // CU
            pic.cus["qp_y"][i] = qp[uy][ux]
            assert not int(c["flags"]), "a generated unit with PCM / bypass set"
            if n_refs == 0 or is_pcm(spec, ux, uy):
                pcm_units.add((ux, uy))
                pic.cus["pred_mode"][i], pic.cus["part_mode"][i], pic.cus["flags"][i] = 0, 0, W.CUF_PCM
                pic.ctbs["flags"][a] |= W.CTBF_HAS_PCM_OR_BYPASS
                for cidx, bx, by, l2 in _pcm_blocks(x, y, cf):
                    ib = np.zeros(1, W.IB)
                    ib["x"], ib["y"], ib["cidx"], ib["log2_size"], ib["mode"], ib["flags"], ib["res_ofs"] = bx, by, cidx, l2, 1, W.IBF_PCM, n_pcm
                    n_pcm += 1 << (2 * l2)
                    ibs.append(ib)
        pic.ctbs["ib_count"][a] = len(ibs) - int(pic.ctbs["ib_start"][a])
    for i, c in enumerate(pic.cus):                       # (the transform leaves stay in the order of the units)
        key = (int(c["x"]) // CU, int(c["y"]) // CU)
        if key in pcm_units:
            t = np.zeros(1, W.TU)
            t["x"], t["y"], t["log2_size"] = c["x"], c["y"], 4
            tus.append(t)
        else:
            tus.append(gen.tus[leaves[key]])
    pic.tus = np.concatenate(tus)
    pic.ibs = np.concatenate(ibs) if ibs else np.zeros(0, W.IB)
    pic.pcm = np.zeros(n_pcm, np.dtype("<u2"))
    keep = [i for i, p in enumerate(pic.pbs) if (int(p["x"]) // CU, int(p["y"]) // CU) not in pcm_units]
    pic.pbs = pic.pbs[keep].copy()
    for i, p in enumerate(pic.pbs):
        slot = ((int(p["x"]) // CU) + (int(p["y"]) // CU)) % n_refs
        pic.pbs["flags"][i] = W.PBF_PRED_L0 | W.PBF_MC_L0
        pic.pbs["ref_slot"][i] = [slot, slot]
        pic.pbs["mv"][i] = 0
        pic.pbs["wt_idx"][i] = 0
    pic.meta = dict(gen.meta, spec=dict(spec))
    return pic


def check_legal(pic):
    """everything rewritten is what a bitstream can carry"""
    pp = pic.pp[0]
    qmin = -6 * (int(pp["bit_depth_luma"]) - 8)
    assert all(qmin <= int(q) <= 51 for q in pic.cus["qp_y"])
    assert -12 <= int(pp["pic_cb_qp_offset"]) <= 12 and -12 <= int(pp["pic_cr_qp_offset"]) <= 12
    for s in pic.slices:
        for name in ("beta_offset", "tc_offset"):
            assert int(s[name]) % 2 == 0 and -12 <= int(s[name]) <= 12      # slice_beta_offset_div2 / slice_tc_offset_div2 in -6..6
    assert not int(pp["flags"]) & W.PF_PCM_LOOP_FILTER_DISABLE
    maxv = [(1 << int(pp["bit_depth_luma"])) - 1] + [(1 << int(pp["bit_depth_chroma"])) - 1] * 2
    for ib in pic.ibs:
        n = 1 << (2 * int(ib["log2_size"]))
        assert int(ib["flags"]) == W.IBF_PCM and int(pic.pcm[int(ib["res_ofs"]):int(ib["res_ofs"]) + n].max()) <= maxv[int(ib["cidx"])]


# ------------------------------------------------------------------------------------------------------------------- the segments
def _qp_map(pic):
    pp = pic.pp[0]
    m = np.zeros((int(pp["height"]) // 4, int(pp["width"]) // 4), np.int64)
    for c in pic.cus:
        n = (1 << int(c["log2_size"])) // 4
        m[int(c["y"]) // 4:int(c["y"]) // 4 + n, int(c["x"]) // 4:int(c["x"]) // 4 + n] = int(c["qp_y"])
    return m


def _slice_map(pic):
    pp = pic.pp[0]
    cs = int(pp["log2_ctb_size"])
    m = np.zeros((int(pp["height"]) // 4, int(pp["width"]) // 4), np.int64)
    for a, ctb in enumerate(pic.ctbs):
        cx, cy = a % pic.pic_w_ctbs, a // pic.pic_w_ctbs
        m[(cy << cs) // 4:((cy + 1) << cs) // 4, (cx << cs) // 4:((cx + 1) << cs) // 4] = int(ctb["slice_idx"])
    return m


def luma_params(s, sc, change=None):
    """(beta, tc) of a luma segment as deblock.cc:517-531 derives them, under one change of the tables (module header)"""
    qpl = (s["qp_q"] + s["qp_p"] + (0 if change == "round" else 1)) >> 1
    bi = clip3(0, 50 if change == "beta_hi" else 51, qpl + s["beta_offset"])
    ti = clip3(0, 52 if change == "tc_hi" else 53, qpl + 2 * (s["bs"] - 1) + s["tc_offset"])
    eb = TAB_BETA[bi] + {"beta-": -1, "beta+": 1}.get(change, 0)
    et = TAB_TC[ti] + {"tc-": -1, "tc+": 1}.get(change, 0)
    return max(0, eb) * sc, max(0, et) * sc


def chroma_qp(qpi, cf):
    if cf == 1:                                                    # table8_22 (transform.h:29-34)
        return qpi if qpi < 30 else (qpi - 6 if qpi >= 43 else TAB_QPC_420[qpi - 30])
    return min(qpi, 51)


def chroma_params(s, c, cf, sc, change=None):
    """tc of plane c (0: Cb, 1: Cr) of a chroma segment as deblock.cc:698-721 derives it, under one change"""
    qpi = ((s["qp_q"] + s["qp_p"] + (0 if change == "round" else 1)) >> 1) + s["c_offset"][c]
    qpc = chroma_qp(qpi, cf) + {"qpc-": -1, "qpc+": 1}.get(change, 0)
    if change == "nomin" and cf != 1:
        qpc = qpi
    ti = clip3(0, 52 if change == "tc_hi" else 53, qpc + 2 * (s["bs"] - 1) + s["tc_offset"])
    return max(0, TAB_TC[ti] + {"tc-": -1, "tc+": 1}.get(change, 0)) * sc


def segments(pic):
    """-> (luma segments with bS > 0, chroma segments with bS 2) with the QPs, offsets, index sums and indices of each; (x, y) is the
    first Q sample in LUMA samples, as bs_reference gives it"""
    pp = pic.pp[0]
    cf = int(pp["chroma_format_idc"])
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    qp, sl = _qp_map(pic), _slice_map(pic)
    luma, chroma = [], []
    for b in bs_reference(pic):
        if b["bs"] == 0:
            continue
        x, y, v = b["x"], b["y"], b["vertical"]
        xp, yp = (x - 1, y) if v else (x, y - 1)
        sh_q = pic.slices[sl[y // 4, x // 4]]
        s = dict(vertical=v, x=x, y=y, bs=b["bs"], qp_q=int(qp[y // 4, x // 4]), qp_p=int(qp[yp // 4, xp // 4]),
                 beta_offset=int(sh_q["beta_offset"]), tc_offset=int(sh_q["tc_offset"]), pcm_side=b["pcm_side"], inter_side=b["inter_side"])
        s["odd"] = bool((s["qp_q"] + s["qp_p"]) & 1)
        s["qpl"] = (s["qp_q"] + s["qp_p"] + 1) >> 1
        s["beta_sum"], s["tc_sum"] = s["qpl"] + s["beta_offset"], s["qpl"] + 2 * (s["bs"] - 1) + s["tc_offset"]
        s["beta_idx"], s["tc_idx"] = clip3(0, 51, s["beta_sum"]), clip3(0, 53, s["tc_sum"])
        along, across = (y, x) if v else (x, y)
        s["directed"] = across % CU == 0 and along % CU in (4, 8)
        luma.append(s)
        # the chroma loop (deblock.cc:660-667) visits the 8-sample chroma grid across and every 4 chroma lines along the edge
        if cf and b["bs"] == 2 and (x % (8 * sw) == 0 if v else y % (8 * sh) == 0) and (y % (4 * sh) == 0 if v else x % (4 * sw) == 0):
            c = dict(s, xc=x // sw, yc=y // sh, c_offset=(int(pp["pic_cb_qp_offset"]), int(pp["pic_cr_qp_offset"])))
            c["qpi"] = [c["qpl"] + o for o in c["c_offset"]]
            c["qpc"] = [chroma_qp(q, cf) for q in c["qpi"]]
            c["ctc_sum"] = [q + 2 + c["tc_offset"] for q in c["qpc"]]
            c["ctc_idx"] = [clip3(0, 53, t) for t in c["ctc_sum"]]
            chroma.append(c)
    return luma, chroma


# --------------------------------------------------------------------------------------------------------------------- the canvas
def canvas(pic, luma):
    """the picture before the filter (module header) -> planes"""
    pp = pic.pp[0]
    w, h, cf = int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"])
    bd, bdc = int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"])
    dt = np.uint8 if bd <= 8 else np.uint16
    sc = 1 << (bd - 8)
    Y = np.full((h, w), 128 * sc, np.int64)
    for s in luma:
        if not s["directed"]:
            continue
        v, x, y = s["vertical"], s["x"], s["y"]
        across, along = (x, y) if v else (y, x)
        eb, et = TAB_BETA[s["beta_idx"]] or 6, TAB_TC[s["tc_idx"]] or 1
        second = along % CU == 8
        ux, uy = x // CU, y // CU
        s["off"] = off = second and bool((ux + uy) & 1)
        d = eb * sc - (0 if off else 1)
        step = -((8 - 16 * (et + 2) * sc) // 6)                     # the smallest step whose delta (6 * step + 8) >> 4 is (tc' + 2) units
        sign = -1 if (ux + uy + int(second) + int(v)) & 1 else 1
        A = 128 * sc - sign * (step // 2)
        B = A + sign * step
        P = np.full((4, 4), A, np.int64)                             # [line][distance from the edge]
        for k in range(4):
            P[k, 2:] = A - sign * ((d + 1) // 2 if k < 3 else d // 2)
        Q = np.full((4, 4), B, np.int64)
        T = Y if v else Y.T
        T[along:along + 4, across - 4:across] = P[:, ::-1]
        T[along:along + 4, across:across + 4] = Q
    assert Y.min() >= 0 and Y.max() < (1 << bd)
    planes = [Y.astype(dt)]
    if cf:
        scc = 1 << (bdc - 8)
        cw, ch = W.plane_dims(w, h, cf)[1]
        sw, sh = w // cw, h // ch
        yy, xx = np.mgrid[0:ch, 0:cw]
        board = ((xx * sw // CU + yy * sh // CU) & 1) * 2 - 1
        C = (128 * scc + board * (CHROMA_STEP // 2) * scc).astype(dt)
        planes += [C, C.copy()]
    return planes


def fill_samples(pic, planes):
    """the PCM units' raw samples from the canvas; -> the references (every slot holds the canvas)"""
    for ib in pic.ibs:
        x, y, n, o = int(ib["x"]), int(ib["y"]), 1 << int(ib["log2_size"]), int(ib["res_ofs"])
        pic.pcm[o:o + n * n] = planes[int(ib["cidx"])][y:y + n, x:x + n].reshape(-1)
    return [[p.copy() for p in planes] for _ in range(int(pic.meta["cfg"]["n_refs"]))]


def qp_picture(spec, **cfg):
    """-> (picture, references, canvas planes, luma segments, chroma segments)"""
    full = dict(BASE, **cfg)
    pic = rewrite_lists(synth.picture(**full), spec)
    luma, chroma = segments(pic)
    planes = canvas(pic, luma)
    refs = fill_samples(pic, planes)
    check_legal(pic)
    return pic, refs, planes, luma, chroma


# ---------------------------------------------------------------------------------------------------------------- the restatement
def filter_luma(p, q, beta, tc, bd):
    """one luma segment (deblock.cc:535-570, fallback-deblk.h:33-98): p, q = [line][distance] -> new (p, q)"""
    p, q = [list(r) for r in p], [list(r) for r in q]
    dp0, dp3 = abs(p[0][2] - 2 * p[0][1] + p[0][0]), abs(p[3][2] - 2 * p[3][1] + p[3][0])
    dq0, dq3 = abs(q[0][2] - 2 * q[0][1] + q[0][0]), abs(q[3][2] - 2 * q[3][1] + q[3][0])
    dpq0, dpq3, dp, dq = dp0 + dq0, dp3 + dq3, dp0 + dp3, dq0 + dq3
    if not dpq0 + dpq3 < beta:
        return p, q
    sam = [2 * dpq < (beta >> 2) and abs(p[k][3] - p[k][0]) + abs(q[k][0] - q[k][3]) < (beta >> 3) and abs(p[k][0] - q[k][0]) < ((5 * tc + 1) >> 1)
           for k, dpq in ((0, dpq0), (3, dpq3))]
    dep, deq = dp < ((beta + (beta >> 1)) >> 3), dq < ((beta + (beta >> 1)) >> 3)
    maxv = (1 << bd) - 1
    for k in range(4):
        p0, p1, p2, p3 = p[k]
        q0, q1, q2, q3 = q[k]
        if sam[0] and sam[1]:
            p[k][0] = clip3(p0 - 2 * tc, p0 + 2 * tc, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3)
            p[k][1] = clip3(p1 - 2 * tc, p1 + 2 * tc, (p2 + p1 + p0 + q0 + 2) >> 2)
            p[k][2] = clip3(p2 - 2 * tc, p2 + 2 * tc, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3)
            q[k][0] = clip3(q0 - 2 * tc, q0 + 2 * tc, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3)
            q[k][1] = clip3(q1 - 2 * tc, q1 + 2 * tc, (p0 + q0 + q1 + q2 + 2) >> 2)
            q[k][2] = clip3(q2 - 2 * tc, q2 + 2 * tc, (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3)
            continue
        delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
        if abs(delta) < tc * 10:
            delta = clip3(-tc, tc, delta)
            p[k][0], q[k][0] = clip3(0, maxv, p0 + delta), clip3(0, maxv, q0 - delta)
            if dep:
                p[k][1] = clip3(0, maxv, p1 + clip3(-(tc >> 1), tc >> 1, (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1))
            if deq:
                q[k][1] = clip3(0, maxv, q1 + clip3(-(tc >> 1), tc >> 1, (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1))
    return p, q


def filter_chroma(p, q, tc, bd):
    """one chroma segment (fallback-deblk.h:103-124): p, q = [line][distance 0..1] -> new (p, q)"""
    p, q = [list(r) for r in p], [list(r) for r in q]
    maxv = (1 << bd) - 1
    for k in range(4):
        delta = clip3(-tc, tc, (((q[k][0] - p[k][0]) * 4) + p[k][1] - q[k][1] + 4) >> 3)
        p[k][0], q[k][0] = clip3(0, maxv, p[k][0] + delta), clip3(0, maxv, q[k][0] - delta)
    return p, q


def _get(T, along, across, n):
    """the segment's samples of the plane T (transposed for horizontal edges) -> p, q as [line][distance]"""
    return ([[int(T[along + k, across - 1 - i]) for i in range(n)] for k in range(4)],
            [[int(T[along + k, across + i]) for i in range(n)] for k in range(4)])


def _put(T, along, across, p, q):
    for k in range(4):
        for i in range(len(p[k])):
            T[along + k, across - 1 - i], T[along + k, across + i] = p[k][i], q[k][i]


def _safe_lines(vertical, along):
    """the lines of a segment that the other pass cannot write: for a vertical edge those 3 and 4 samples from the horizontal grid lines (the
    horizontal pass writes up to 3 luma samples and 1 chroma sample beside them); the horizontal pass is the last one"""
    return [k for k in range(4) if (along + k) % 8 in (3, 4)] if vertical else [0, 1, 2, 3]


def restate(pic, planes, luma, chroma):
    """the planes after the deblocking stage, from `planes` before it.  Sets on every segment `live` (its output differs from its input) and
    `sens` (the changes its output is sensitive to); chroma segments hold a list of two, Cb and Cr, and `planes_differ`"""
    pp = pic.pp[0]
    cf, bd, bdc = int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"])
    sc, scc = 1 << (bd - 8), 1 << (bdc - 8)
    out = [p.astype(np.int64) for p in planes]
    for vertical in (True, False):
        T = [o if vertical else o.T for o in out]
        for s in luma:
            if s["vertical"] != vertical:
                continue
            along, across = (s["y"], s["x"]) if vertical else (s["x"], s["y"])
            p, q = _get(T[0], along, across, 4)
            base = filter_luma(p, q, *luma_params(s, sc), bd)
            lines = _safe_lines(vertical, along)
            s["live"] = any(base[0][k] != p[k] or base[1][k] != q[k] for k in lines)
            s["sens"] = set()
            for ch in LUMA_CHANGES:
                alt = filter_luma(p, q, *luma_params(s, sc, ch), bd)
                if any(alt[0][k] != base[0][k] or alt[1][k] != base[1][k] for k in lines):
                    s["sens"].add(ch)
            _put(T[0], along, across, *base)
        for s in chroma:
            if s["vertical"] != vertical:
                continue
            along, across = (s["yc"], s["xc"]) if vertical else (s["xc"], s["yc"])
            s["live"], s["sens"], res = [], [], []
            # the horizontal chroma pass writes one sample beside the grid lines: lines 1 and 2 of a vertical segment are out of its reach
            lines = [1, 2] if vertical else [0, 1, 2, 3]
            for c in (0, 1):
                p, q = _get(T[1 + c], along, across, 2)
                base = filter_chroma(p, q, chroma_params(s, c, cf, scc), bdc)
                s["live"].append(any(base[0][k] != p[k] or base[1][k] != q[k] for k in lines))
                sens = set()
                for ch in CHROMA_CHANGES:
                    alt = filter_chroma(p, q, chroma_params(s, c, cf, scc, ch), bdc)
                    if any(alt[0][k] != base[0][k] or alt[1][k] != base[1][k] for k in lines):
                        sens.add(ch)
                s["sens"].append(sens)
                res.append([base[0][k][0] - p[k][0] for k in lines])
                _put(T[1 + c], along, across, *base)
            s["planes_differ"] = res[0] != res[1]                 # what the filter added to p0 differs between Cb and Cr
    return [o.astype(p.dtype) for o, p in zip(out, planes)]


# ---------------------------------------------------------------------------------------------------------------------- the census
def census(made):
    """made: list of (picture, luma segments, chroma segments) after restate() -> the counts that check_census() asks for"""
    cen = dict(beta={}, tc={}, low_beta=[0, 0], low_tc=[0, 0], beta_neg=0, tc_neg=0, beta_over=[0, 0], tc_over=[0, 0], odd=[0, 0], even=0,
               off_on=[0, 0], bs=[0, 0, 0], qpl_neg=0, chroma=[{}, {}], c_neg=[[0, 0], [0, 0]], c_nomin=[0, 0], planes_differ=0, c_odd=0)
    for pic, luma, chroma in made:
        pp = pic.pp[0]
        cb, cr = int(pp["pic_cb_qp_offset"]), int(pp["pic_cr_qp_offset"])
        opposite = cb * cr < 0 and abs(cb) != abs(cr)
        for s in luma:
            v = s["vertical"]
            cen["bs"][s["bs"]] += 1
            if s["sens"] & {"beta-", "beta+"}:
                cen["beta"][(s["beta_idx"], v)] = cen["beta"].get((s["beta_idx"], v), 0) + 1
                cen["off_on"][0 if s["live"] else 1] += 1
            if s["sens"] & {"tc-", "tc+"}:
                cen["tc"][(s["tc_idx"], v)] = cen["tc"].get((s["tc_idx"], v), 0) + 1
            if s["beta_idx"] <= 15:
                cen["low_beta"][0] += 1
                cen["low_beta"][1] += int(s["live"])
            if s["tc_idx"] <= 17:
                cen["low_tc"][0] += 1
                cen["low_tc"][1] += int(s["live"])
            cen["beta_neg"] += int(s["beta_sum"] < 0)
            cen["qpl_neg"] += int(s["qpl"] < 0)
            cen["tc_neg"] += int(s["tc_sum"] < 0)
            if s["beta_sum"] > 51:
                cen["beta_over"][0] += 1
                cen["beta_over"][1] += int("beta_hi" in s["sens"])
            if s["tc_sum"] > 53:
                cen["tc_over"][0] += 1
                cen["tc_over"][1] += int("tc_hi" in s["sens"])
            if s["odd"]:
                cen["odd"][0] += int(bool(s["sens"]))
                cen["odd"][1] += int("round" in s["sens"])
            else:
                cen["even"] += int(bool(s["sens"]))
        for s in chroma:
            for c in (0, 1):
                qpi = s["qpi"][c]
                if qpi < 0:
                    cen["c_neg"][c][0] += 1
                    cen["c_neg"][c][1] += int(s["live"][c])
                if s["sens"][c] & {"qpc-", "qpc+"}:
                    cen["chroma"][c][qpi] = cen["chroma"][c].get(qpi, 0) + 1
                cen["c_nomin"][c] += int(qpi > 51 and "nomin" in s["sens"][c])
            cen["planes_differ"] += int(opposite and s["planes_differ"])
            cen["c_odd"] += int(s["odd"] and ("round" in s["sens"][0] or "round" in s["sens"][1]))
    return cen


def census_failures(cen, cf, bd=8, check_luma=True):
    """the conditions of tests/test_deblock_qp_range.py's header that do not hold -> list of texts"""
    bad = []
    if bd > 8 and cen["qpl_neg"] < 8:
        bad.append("a negative QP average in %d segments" % cen["qpl_neg"])
    if check_luma:
        for v in (True, False):
            missing = [i for i in range(16, 52) if cen["beta"].get((i, v), 0) < 2]
            if missing:
                bad.append("beta indices %s in fewer than 2 sensitive segments (vertical %s)" % (missing, v))
            missing = [i for i in range(18, 54) if cen["tc"].get((i, v), 0) < 2]
            if missing:
                bad.append("tc indices %s in fewer than 2 sensitive segments (vertical %s)" % (missing, v))
        for name in ("low_beta", "low_tc"):
            if cen[name][0] < 8 or cen[name][1]:
                bad.append("%s: %d segments, %d not silent" % (name, cen[name][0], cen[name][1]))
        for name in ("beta_neg", "tc_neg"):
            if cen[name] < 2:
                bad.append("%s: %d segments" % (name, cen[name]))
        for name in ("beta_over", "tc_over"):
            if cen[name][1] < 2:
                bad.append("%s: %d segments, %d sensitive to the bound" % (name, cen[name][0], cen[name][1]))
        if cen["odd"][1] < 8 or cen["even"] < 8:
            bad.append("sensitive segments at odd QP sums %d (to the rounding: %d), at even sums %d" % (cen["odd"][0], cen["odd"][1], cen["even"]))
        if min(cen["off_on"]) < 8:
            bad.append("segments sensitive to beta that are on / off: %s" % cen["off_on"][::-1])
    for c in (0, 1) if cf else ():
        n = cen["chroma"][c]
        if cf == 1:
            missing = [q for q in range(30, 43) if n.get(q, 0) < 2]
            if missing:
                bad.append("plane %d: qP_i %s in fewer than 2 sensitive segments" % (c + 1, missing))
            hi, lo = sum(k for q, k in n.items() if q >= 43), sum(k for q, k in n.items() if q < 30)
            if hi < 4 or n.get(43, 0) < 2:
                bad.append("plane %d: qP_i >= 43 in %d sensitive segments, 43 in %d" % (c + 1, hi, n.get(43, 0)))
            if lo < 4 or n.get(29, 0) < 2:
                bad.append("plane %d: qP_i < 30 in %d sensitive segments, 29 in %d" % (c + 1, lo, n.get(29, 0)))
            if cen["c_neg"][c][0] < 2 or cen["c_neg"][c][1]:
                bad.append("plane %d: negative qP_i in %d segments, %d not silent" % (c + 1, cen["c_neg"][c][0], cen["c_neg"][c][1]))
        else:
            if cen["c_nomin"][c] < 4:
                bad.append("plane %d: qP_i 52..63 in %d segments sensitive to the min" % (c + 1, cen["c_nomin"][c]))
            for q in (50, 51):
                if n.get(q, 0) < 2:
                    bad.append("plane %d: qP_i %d in %d sensitive segments" % (c + 1, q, n.get(q, 0)))
    if cf:
        if cen["planes_differ"] < 8:
            bad.append("Cb and Cr filter differently in %d segments of pictures with opposite offsets" % cen["planes_differ"])
        if cen["c_odd"] < 8:
            bad.append("chroma segments at odd QP sums sensitive to the rounding: %d" % cen["c_odd"])
    return bad


def census_line(cid, cen, cf):
    def least(d, lo, hi, v):
        return min(d.get((i, v), 0) for i in range(lo, hi))
    line = "%-14s beta %d/%d tc %d/%d | low %d, %d | <0 %d, %d | over %d/%d, %d/%d | odd %d (%d), even %d | on %d off %d | bS 1: %d, 2: %d | QP < 0 %d" % (
        cid, least(cen["beta"], 16, 52, True), least(cen["beta"], 16, 52, False), least(cen["tc"], 18, 54, True), least(cen["tc"], 18, 54, False),
        cen["low_beta"][0], cen["low_tc"][0], cen["beta_neg"], cen["tc_neg"], cen["beta_over"][1], cen["beta_over"][0], cen["tc_over"][1],
        cen["tc_over"][0], cen["odd"][0], cen["odd"][1], cen["even"], cen["off_on"][0], cen["off_on"][1], cen["bs"][1], cen["bs"][2], cen["qpl_neg"])
    for c in (0, 1) if cf else ():
        n = cen["chroma"][c]
        if cf == 1:
            line += " | %s tab %d, >=43 %d (43: %d), <30 %d (29: %d), <0 %d" % ("Cb" if c == 0 else "Cr", min(n.get(q, 0) for q in range(30, 43)),
                                                                                sum(k for q, k in n.items() if q >= 43), n.get(43, 0),
                                                                                sum(k for q, k in n.items() if q < 30), n.get(29, 0), cen["c_neg"][c][0])
        else:
            line += " | %s min %d, 51: %d, 50: %d" % ("Cb" if c == 0 else "Cr", cen["c_nomin"][c], n.get(51, 0), n.get(50, 0))
    if cf:
        line += " | Cb != Cr %d, odd %d" % (cen["planes_differ"], cen["c_odd"])
    return line
