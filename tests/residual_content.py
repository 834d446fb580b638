"""Content that lets the residual and intra stages SHOW what they computed, and a census of what reached the picture
(tests/test_residual_inrange.py, tests/test_intra_strong.py).

The generator's coefficient blocks (csrc/synth.c gen_coeffs: sparse +-512, dense +-2048, full int16, at QP 22..37) dequantise to residuals
several times the sample range: most samples a residual block writes leave the range before the final Clip(pred + r), and intra blocks then
predict from borders made of 0 and maxv.  A wrong low bit of a butterfly, of a rounding term or of an interpolation weight is invisible there.

  * attenuate_levels() divides the magnitude of every level (not those of cu_transquant_bypass blocks, which are +-40 already) by 1 << shift:
    sparse and dense blocks land inside the range, the full-int16 blocks still saturate, so both regimes stay in one picture;
  * axis_ramp_refs() replaces the reference planes by a ramp along ONE axis (smooth_refs of deblock_content.py slopes in both, which makes the
    left-border flatness test of a 32x32 block fail whenever its below-left neighbour is substituted);
  * residual_census() / border_census() / strong_census() classify what happened from the lists and the oracle's planes alone: no kernel gets
    a counter."""
import numpy as np

from libde265_amd import worklist as W

# the level shift per luma depth of the cases (chosen on the oracle's census): what a level is worth in samples falls with the depth, as the
# dequantiser's bdShift grows with it.  At 16 bits the sparse blocks fit as they are; 2 brings the dense +-2048 blocks inside as well
SHIFT = {8: 7, 9: 6, 10: 6, 12: 5, 16: 2}


def attenuate_levels(pic, shift, prescaled_shift=None):
    """a copy of pic whose levels have the magnitude max(1, |level| >> shift): sign and position kept, bypass blocks untouched, narrow blocks
    stay narrow (a smaller level still fits 8 bits).  prescaled_shift: another shift for the blocks with RBF_DEQUANTIZED, whose levels are
    coefficients already and skip the dequantiser's gain"""
    entries, n = W._wide_entries(pic)
    lvl = (entries >> 16).astype(np.uint16).view(np.int16).astype(np.int64)
    keep = np.repeat(pic.rbs["kind"] == W.RK_BYPASS, n)
    pre = np.repeat((pic.rbs["flags"] & W.RBF_DEQUANTIZED) != 0, n)
    mag = np.maximum(1, np.abs(lvl) >> np.where(pre, shift if prescaled_shift is None else prescaled_shift, shift))
    new = np.where(keep, lvl, np.where(lvl < 0, -mag, mag))
    entries = ((entries & 0xFFFF) | ((new & 0xFFFF).astype(np.uint32) << 16)).astype(np.uint32)
    return W._relayout(pic, entries, n, (pic.rbs["flags"] & W.RBF_NARROW) != 0)


def axis_ramp_plane(h, w, bd, axis, dtype):
    """1/2 of an 8-bit step per sample along `axis` ("x" or "y") from a quarter of the range; the coordinate folds back every 256 samples
    (a triangle), so the plane stays within [1/4, 3/4] of the range at any size"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    t = (xx if axis == "x" else yy) & 511
    t = np.where(t < 256, t, 511 - t)
    return ((1 << bd) // 4 + ((t << (bd - 8)) >> 1)).astype(dtype)


def axis_ramp_refs(refs, bd_luma, bd_chroma, axis):
    """the reference planes replaced by axis_ramp_plane"""
    return [[axis_ramp_plane(p.shape[0], p.shape[1], bd_chroma if c else bd_luma, axis, p.dtype) for c, p in enumerate(planes)] for planes in refs]


def _bd(pp, c):
    return int(pp["bit_depth_chroma" if c else "bit_depth_luma"])


def _tally(t, log2, a, maxv, pred=None):
    e = t.setdefault(log2, dict(samples=0, unclipped=0, changed=0, at_min=0, at_max=0, blocks=0, clip_free=0))
    inside = (a > 0) & (a < maxv)
    e["samples"] += a.size
    e["unclipped"] += int(inside.sum())
    e["at_min"] += int((a == 0).sum())
    e["at_max"] += int((a == maxv).sum())
    e["blocks"] += 1
    e["clip_free"] += int(inside.all())
    if pred is not None:
        e["changed"] += int((a != pred).sum())


def residual_census(pred_planes, recon_planes, pic, intra_planes=None):
    """pred_planes: the oracle with STAGE_INTER alone; recon_planes: with INTER | RESIDUAL; intra_planes: with INTER | RESIDUAL | INTRA.
    -> dict(inter={log2: counts}, intra={log2: counts}) over the residual blocks that are not deferred / the intra blocks with a residual:
    samples, unclipped (0 < recon < maxv: conservative, a sample that lands on 0 or maxv without the clip counts as clipped), at_min / at_max,
    changed (recon != pred; inter only: an intra block's prediction never reaches a plane), blocks, clip_free (every sample unclipped)"""
    pp = pic.pp[0]
    out = dict(inter={}, intra={})
    for rb in pic.rbs[(pic.rbs["flags"] & W.RBF_DEFERRED) == 0]:
        c, x, y, l2 = int(rb["cidx"]), int(rb["x"]), int(rb["y"]), int(rb["log2_size"])
        n = 1 << l2
        _tally(out["inter"], l2, recon_planes[c][y:y + n, x:x + n], (1 << _bd(pp, c)) - 1, pred_planes[c][y:y + n, x:x + n])
    if intra_planes is not None:
        for ib in pic.ibs[(pic.ibs["flags"] & W.IBF_HAS_RESIDUAL) != 0]:
            c, x, y, l2 = int(ib["cidx"]), int(ib["x"]), int(ib["y"]), int(ib["log2_size"])
            n = 1 << l2
            _tally(out["intra"], l2, intra_planes[c][y:y + n, x:x + n], (1 << _bd(pp, c)) - 1)
    return out


def border_census(recon_planes, pic):
    """intra blocks of 8x8 and larger (not PCM): dict(blocks, single: the row above and the column to the left, where inside the picture,
    hold ONE value, extreme: ... which is 0 or maxv)"""
    pp = pic.pp[0]
    out = dict(blocks=0, single=0, extreme=0)
    for ib in pic.ibs[(pic.ibs["log2_size"] >= 3) & ((pic.ibs["flags"] & W.IBF_PCM) == 0)]:
        c, x, y, n = int(ib["cidx"]), int(ib["x"]), int(ib["y"]), 1 << int(ib["log2_size"])
        p = recon_planes[c]
        parts = ([p[y - 1, x:x + n]] if y else []) + ([p[y:y + n, x - 1]] if x else [])
        out["blocks"] += 1
        if not parts:
            continue
        b = np.concatenate(parts)
        if (b == b[0]).all():
            out["single"] += 1
            out["extreme"] += int(b[0] == 0 or b[0] == (1 << _bd(pp, c)) - 1)
    return out


def strong_geometry_ok(pic):
    """what strong_census' availability rule needs: one slice, one tile, no constrained intra prediction, CTBs of 32 or 64, CUs of 32x32,
    a picture that is whole CTBs"""
    pp = pic.pp[0]
    cs = pic.ctb_size
    return (len(pic.slices) == 1 and int(pp["num_tile_cols"]) == 1 and int(pp["num_tile_rows"]) == 1 and
            not (int(pp["flags"]) & W.PF_CONSTRAINED_INTRA_PRED) and cs in (32, 64) and bool((pic.cus["log2_size"] == 5).all()) and
            int(pp["width"]) % cs == 0 and int(pp["height"]) % cs == 0)


def _border_32(luma, x, y, w, h, ctb, bd):
    """border[i + 64], i = -64..64, of the 32x32 luma block at (x, y) as the reference gathers it (intrapred.h fill_from_image +
    reference_sample_substitution) when every 32x32 quadrant is one CU: B(0) the corner, B(i) = (x - 1 + i, y - 1), B(-i) = (x - 1, y - 1 + i)"""
    in64 = ctb == 64
    qx, qy = (x >> 5) & 1, (y >> 5) & 1                       # quadrant inside a 64-CTB
    if in64:
        # above-right: the CTB above (TL), the CTB above-right (TR), the CTB's own TR quadrant (BL); the right CTB is later (BR)
        ar = (y > 0 and x + 32 < w) if qy == 0 else qx == 0
        bl = qx == 0 and qy == 0 and x > 0                    # the left CTB's BR quadrant
    else:
        ar = y > 0 and x + 32 < w
        bl = False                                            # the next CTB row is later
    b = np.zeros(129, np.int64)
    ok = np.zeros(129, bool)
    if x > 0 and y > 0:
        b[64], ok[64] = luma[y - 1, x - 1], True
    if y > 0:
        b[65:97], ok[65:97] = luma[y - 1, x:x + 32], True
        if ar:
            b[97:129], ok[97:129] = luma[y - 1, x + 32:x + 64], True
    if x > 0:
        b[63:31:-1], ok[63:31:-1] = luma[y:y + 32, x - 1], True
        if bl and y + 32 < h:
            b[31::-1][:32], ok[31::-1][:32] = luma[y + 32:y + 64, x - 1], True
    if not ok.any():
        b[:] = 1 << (bd - 1)
        return b
    if not ok[0]:
        b[0] = b[np.argmax(ok)]
    for i in range(1, 129):
        if not ok[i]:
            b[i] = b[i - 1]
    return b


def strong_census(recon_planes, pic):
    """32x32 luma intra blocks whose border is filtered (mode not DC, 10 or 26; no PCM) in a picture with PF_STRONG_INTRA_SMOOTHING and without
    PF_INTRA_SMOOTHING_DISABLED (strong_geometry_ok must hold): the two flatness tests of intrapred.h:216-234 recomputed from the planes after the
    intra stage -> dict(candidates, strong, sloped_above / sloped_left (strong with |B(+-64) - B(0)| >= threshold), one_only (one test passes),
    near_miss (fails, both sums below twice the threshold), filtered_121 (candidates that take [1 2 1]), blocks = [(x, y)] of the strong ones)"""
    assert strong_geometry_ok(pic)
    pp = pic.pp[0]
    w, h, bd = int(pp["width"]), int(pp["height"]), int(pp["bit_depth_luma"])
    out = dict(candidates=0, strong=0, sloped_above=0, sloped_left=0, one_only=0, near_miss=0, filtered_121=0, blocks=[])
    fl = int(pp["flags"])
    if not (fl & W.PF_STRONG_INTRA_SMOOTHING) or (fl & W.PF_INTRA_SMOOTHING_DISABLED):
        return out
    thr = 1 << (bd - 5)
    sel = (pic.ibs["cidx"] == 0) & (pic.ibs["log2_size"] == 5) & ((pic.ibs["flags"] & W.IBF_PCM) == 0)
    for ib in pic.ibs[sel]:
        if int(ib["mode"]) in (1, 10, 26):
            continue
        x, y = int(ib["x"]), int(ib["y"])
        b = _border_32(recon_planes[0], x, y, w, h, pic.ctb_size, bd)
        sa, sl = abs(b[64] + b[128] - 2 * b[96]), abs(b[64] + b[0] - 2 * b[32])
        out["candidates"] += 1
        if sa < thr and sl < thr:
            out["strong"] += 1
            out["blocks"].append((x, y))
            out["sloped_above"] += int(abs(b[128] - b[64]) >= thr)
            out["sloped_left"] += int(abs(b[0] - b[64]) >= thr)
        else:
            out["filtered_121"] += 1
            out["one_only"] += int((sa < thr) != (sl < thr))
            out["near_miss"] += int(sa < 2 * thr and sl < 2 * thr)
    return out


def differing_blocks_32(a, b):
    """the 32x32 luma blocks [(x, y)] in which the luma planes a and b differ"""
    d = a != b
    h, w = d.shape
    return [(x, y) for y in range(0, h, 32) for x in range(0, w, 32) if d[y:y + 32, x:x + 32].any()]


def check_strong_against_oracle(with_flag, without_flag, pic, cen):
    """The census is trusted only where the oracle agrees: decoded with PF_STRONG_INTRA_SMOOTHING cleared, the picture may change in the blocks
    the census calls strong, and from there on in intra blocks that predict from a changed neighbour (left, above-left, above, above-right,
    below-left); chroma never changes (strong smoothing is luma only).  Every changed block that has NO changed neighbour it could have read must
    be one of the census' strong blocks.  -> (changed blocks, of which strong, strong blocks that did not change: the two filters coincide)"""
    for c in range(1, len(with_flag)):
        assert np.array_equal(with_flag[c], without_flag[c]), "clearing strong intra smoothing changed chroma plane %d" % c
    diff = set(differing_blocks_32(with_flag[0], without_flag[0]))
    strong = set(cen["blocks"])
    intra = set((int(cu["x"]), int(cu["y"])) for cu in pic.cus[pic.cus["pred_mode"] == 0])
    for (x, y) in sorted(diff):
        assert (x, y) in intra, "an inter block at (%d, %d) changed with strong intra smoothing cleared" % (x, y)
        if (x, y) in strong:
            continue
        src = [(x - 32, y), (x - 32, y - 32), (x, y - 32), (x + 32, y - 32), (x - 32, y + 32)]
        assert any(s in diff for s in src), "block (%d, %d) changed with strong intra smoothing cleared; the census does not call it strong" % (x, y)
    return len(diff), len(diff & strong), len(strong - diff)


def free_ctbs(pic):
    """CTB addresses (raster) that hold intra CUs while none of their eight neighbours holds one: no block of theirs can read an intra sample of
    another CTB and nobody reads theirs, whatever the modes (a sufficient condition for the runtime's dependency-free CTBs)"""
    cs, cw, ch = pic.ctb_size, pic.pic_w_ctbs, pic.pic_h_ctbs
    has = np.zeros((ch + 2, cw + 2), bool)
    for cu in pic.cus[pic.cus["pred_mode"] == 0]:
        has[int(cu["y"]) // cs + 1, int(cu["x"]) // cs + 1] = True
    out = []
    for cy in range(ch):
        for cx in range(cw):
            if has[cy + 1, cx + 1] and has[cy:cy + 3, cx:cx + 3].sum() == 1:
                out.append(cy * cw + cx)
    return out
