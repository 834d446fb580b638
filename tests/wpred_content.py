"""Explicit weights whose results stay IN RANGE, and a census of what reached the picture (tests/test_wpred_inrange.py).

The generator (csrc/synth.c gen_pb) draws w = 2^denom + U[-128, 127] for every denominator 0..7 and o = U[-128, 127] << (bd - 8): the legal
range of the bitstream, in which a gain w / 2^denom lies in the tens for the small denominators and is negative for a third of the records.
Four of five luma samples of a weighted prediction block are then 0 or maxv, and at denominators 0..3 the write-back

    one list :  Clip(((s w + 2^(log2WD - 1)) >> log2WD) + o)                       log2WD = denom + max(2, 14 - bd)
    two lists:  Clip((s0 w0 + s1 w1 + ((o0 + o1 + 1) << log2WD)) >> (log2WD + 1))

is compared on the clip alone: a wrong rounding term or a dropped offset is invisible there.

  * inrange_weights() rewrites the weight records of a generated picture, denominators cycled over 0..7, weights inside the legal range with a
    total gain near or below 1 (one list: -1 .. 1.25; two lists: w0 from -1 to 3 with w1 ~ 2 - w0, extrapolation to interpolation) and offsets
    that map mid-grey to mid-grey; every sixth PB grazes an end of the range instead, which keeps the clip exercised;
  * corner_weights() puts the ENDS of the legal ranges that can still land in range (denominators 5..7) on the weighted PBs in turn, on
    references dimmed by dim_refs() so that a gain of 3..5 fits;
  * weighted_census() / corner_census() classify what happened from the lists and the decoded planes alone: no kernel gets a counter."""
import numpy as np

from libde265_amd import worklist as W

CORNER_KINDS = ("w_max", "w_min", "w_zero_alone", "w_zero_of_two", "o_min", "o_max", "osum_min", "osum_max", "opposite")
# corner kinds in the order corner_weights() deals them out, for PBs of one list and of two
_UNI_KINDS = ("w_max", "w_min", "w_zero_alone", "o_min", "o_max")
_BI_KINDS = ("w_max", "w_min", "w_zero_of_two", "osum_min", "osum_max", "opposite")
# the denominators a corner kind can use and still land in range: 2^d - 128 is 0 at d = 7 (a constant block), -w = -(2^d + k) is legal only while
# 2^d + k <= 128 - 2^d, and an offset of -128 needs a gain of 4..5 on the dimmed references, which only d = 5 allows
_KIND_DENOMS = {"w_min": (5, 6), "o_max": (5, 6), "opposite": (5, 6), "o_min": (5,), "osum_min": (5,)}


def _depths(pic):
    pp = pic.pp[0]
    return int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"])


def _sub(pic):
    """(horizontal, vertical) subsampling of the chroma planes"""
    cf = int(pic.pp[0]["chroma_format_idc"])
    return (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)


def _lists(pb):
    return [l for l in range(2) if int(pb["flags"]) & (W.PBF_PRED_L0 << l)]


def weighted_pbs(pic):
    """indices of the PBs with explicit weights"""
    return [int(i) for i in np.nonzero((pic.pbs["flags"] & W.PBF_WEIGHTED) != 0)[0]]


def _clamp(v, lo, hi):
    return max(lo, min(hi, int(v)))


def _store(pic, pb, l, k, w, o8, bd):
    """weight and offset (in units of an 8-bit sample) of list l, component k"""
    wt = pic.wts[int(pb["wt_idx"][l])]
    wt["w"][k] = w
    wt["o"][k] = o8 * (1 << (bd - 8))


def _store_denoms(pic, pb, dl, dc):
    bdl, bdc = _depths(pic)
    for l in range(2):
        wt = pic.wts[int(pb["wt_idx"][l])]
        wt["log2wd_luma"] = dl + max(2, 14 - bdl)
        wt["log2wd_chroma"] = dc + max(2, 14 - bdc)


def _check_private_records(pic, idx):
    """every weighted PB owns its two records (the generator pushes a pair per PB): rewriting one PB's weights cannot change another's"""
    used = np.concatenate([pic.pbs["wt_idx"][i] for i in idx]) if idx else np.zeros(0, np.int64)
    assert len(set(used.tolist())) == 2 * len(idx), "weight records are shared between PBs"


def _graze_offset(content, inside=0):
    """the offset (units of an 8-bit sample) that puts `content` `inside` above 0 or below maxv, whichever a legal offset reaches"""
    return round(inside - content) if content < 128 else round(255 - inside - content)


def inrange_weights(pic, seed):
    """rewrites pic.wts IN PLACE for every PB with PBF_WEIGHTED and returns pic.  Luma denominators cycle 0..7 over the PBs of one list and over
    those of two lists separately (so every (lists, denominator) class fills; fewer denominators where a picture has under 16 PBs of a kind),
    chroma denominators run through another cycle (3 n + 5).  One list: w from -2^d (-2^d / 2 on bright content) to 1.25 * 2^d; two lists: w0
    from -2^d to 3 * 2^d, w1 ~ 2 * 2^d - w0; offsets map mid-grey to mid-grey, all inside the legal range.  Every sixth PB takes a gain near 1
    and an offset that puts its content on an END of the range, so that the clip stays exercised where it decides between neighbouring values.
    The record of the list that a one-list PB does not use gets other legal values, so that reading the wrong record shows"""
    rng = np.random.default_rng(seed)
    bdl, bdc = _depths(pic)
    idx = weighted_pbs(pic)
    _check_private_records(pic, idx)
    total = [sum(len(_lists(pic.pbs[i])) == 1 for i in idx), sum(len(_lists(pic.pbs[i])) == 2 for i in idx)]
    # a picture of a few PBs (64x64 CUs, 16x64 samples) cycles over fewer denominators, spread over 0..7, so that every class still gets two PBs
    period = [max(1, min(8, t // 2)) for t in total]
    scale = [_gain_scale(bd) for bd in (bdl, bdc, bdc)]
    count = [0, 0]
    for nth, i in enumerate(idx):
        pb = pic.pbs[i]
        used = _lists(pb)
        bi = len(used) == 2
        n = count[bi]
        count[bi] += 1
        dl, dc = (n % period[bi]) * 8 // period[bi], (3 * n + 5) % 8
        # every sixth PB grazes an end of the range: the offset puts the block's expected content (_local_mean) on 0 or on maxv, so that about
        # half of its samples clip
        graze = nth % 6 == 5
        m = _local_mean(pic, pb, used, 0)
        _store_denoms(pic, pb, dl, dc)
        for k in range(3):
            d, bd = (dc, bdc) if k else (dl, bdl)
            u = 1 << d
            lo, hi = u - 128, u + 127
            if bi:
                w0 = int(rng.integers(max(lo, -u), min(hi, 3 * u) + 1))
                w1 = _clamp(2 * u - w0 + int(rng.integers(-(u // 4), u // 4 + 1)), lo, hi)
                if graze:
                    w0 = int(rng.integers(u // 2, u + u // 2 + 1))
                    w1 = 2 * u - w0
                # (o0 + o1 + 1) / 2 lifts mid-grey back to mid-grey
                osum = _clamp(round(256 * (1 - scale[k] * (w0 + w1) / (2 * u))) + int(rng.integers(-16, 17)), -256, 254)
                if graze:
                    osum = _clamp(2 * _graze_offset(scale[k] * (w0 + w1) / (2 * u) * m), -256, 254)
                o1 = _clamp(osum - _clamp(osum // 2 + int(rng.integers(-20, 21)), -128, 127), -128, 127)
                o0 = _clamp(osum - o1, -128, 127)
                _store(pic, pb, 0, k, w0, o0, bd)
                _store(pic, pb, 1, k, w1, o1, bd)
            else:
                # (an offset ends at 127: under a gain of -1 only the darker half of the range comes back into it)
                w = int(rng.integers(max(lo, -u if m < 110 else -(u // 2)), min(hi, 5 * u // 4) + 1))
                if graze:
                    w = int(rng.integers(u, 5 * u // 4 + 1))
                o = _clamp(round(128 * (1 - scale[k] * w / u)) + int(rng.integers(-8, 9)), -128, 127)
                if graze:
                    o = _clamp(_graze_offset(scale[k] * w / u * m), -128, 127)
                _store(pic, pb, used[0], k, w, o, bd)
                _store(pic, pb, 1 - used[0], k, int(rng.integers(lo, hi + 1)), int(rng.integers(-128, 128)), bd)
    return pic


def dim_refs(refs, shift):
    """the reference planes shifted right: a gain of 1 << shift and more still lands in range"""
    return [[(p >> shift).astype(p.dtype) for p in planes] for planes in refs]


def _local_mean(pic, pb, used, dim):
    """what the generator's reference planes hold around the block a PB predicts from, in units of an 8-bit sample: synth.c
    m355_synth_ref_plane is blurred noise of mean 1/4 of the range on a diagonal ramp from 0 to 1/2 of it (corner_census asserts the outcome,
    so a change there cannot empty the test unnoticed)"""
    pp = pic.pp[0]
    width, height = int(pp["width"]), int(pp["height"])
    cx = int(pb["x"]) + int(pb["w"]) / 2 + sum(int(pb["mv"][l][0]) for l in used) / (4 * len(used))
    cy = int(pb["y"]) + int(pb["h"]) / 2 + sum(int(pb["mv"][l][1]) for l in used) / (4 * len(used))
    t = min(1.0, max(0.0, (cx + cy) / (width + height)))
    return (64 + 128 * t) / (1 << dim)


def corner_weights(pic, seed, dim=2):
    """rewrites pic.wts IN PLACE and returns pic: the kinds of CORNER_KINDS dealt round-robin over the weighted PBs of one list (_UNI_KINDS) and of
    two lists (_BI_KINDS), the same kind in all three components (w_zero_alone: luma only, a block of w = 0 and one list is the constant o; its
    chroma keeps a gain of 1), denominators 5..7 cycled per kind.  What a kind leaves free — the offset under a pinned weight, the weight under a
    pinned offset — is chosen so that the block's expected content (_local_mean of references dimmed by `dim`) lands mid-range"""
    rng = np.random.default_rng(seed)
    bdl, bdc = _depths(pic)
    idx = weighted_pbs(pic)
    _check_private_records(pic, idx)
    count = [0, 0]
    for i in idx:
        pb = pic.pbs[i]
        used = _lists(pb)
        bi = len(used) == 2
        n = count[bi]
        count[bi] += 1
        kinds = _BI_KINDS if bi else _UNI_KINDS
        kind, turn = kinds[n % len(kinds)], n // len(kinds)
        dens = _KIND_DENOMS.get(kind, (5, 6, 7))
        dl, dc = dens[turn % len(dens)], dens[(turn + 1) % len(dens)]
        _store_denoms(pic, pb, dl, dc)
        m = _local_mean(pic, pb, used, dim)
        for k in range(3):
            d, bd = (dc, bdc) if k else (dl, bdl)
            u = 1 << d
            lo, hi = u - 128, u + 127
            jit = int(rng.integers(-4, 5))
            if not bi:
                if kind == "w_max":
                    w = hi
                    o = 128 - w * m / u
                elif kind == "w_min":
                    w = lo
                    o = 128 - w * m / u
                elif kind == "w_zero_alone":
                    w = 0 if k == 0 else u
                    o = int(rng.integers(16, 112)) if k == 0 else 128 - m
                elif kind == "o_min":
                    o = -128 - jit
                    w = _clamp(round(u * (56 + 128) / m), lo, hi)
                else:                                                     # o_max
                    o = 127 - jit
                    w = _clamp(round(u * (64 - 127) / m), lo, hi)
                _store(pic, pb, used[0], k, w, _clamp(round(o) + jit, -128, 127), bd)
                _store(pic, pb, 1 - used[0], k, int(rng.integers(lo, hi + 1)), int(rng.integers(-128, 128)), bd)
                continue
            first = turn & 1                                              # the list that carries the pinned weight
            if kind in ("w_max", "w_min"):
                wa = hi if kind == "w_max" else lo
                wb = _clamp(2 * u - wa, lo, hi)
                osum = 2 * (128 - m * (wa + wb) / (2 * u))
            elif kind == "w_zero_of_two":
                wa, wb = 0, _clamp(2 * u, lo, hi)
                osum = 2 * (128 - m * wb / (2 * u))
            elif kind == "osum_min":
                wa = wb = _clamp(round(u * (56 + 128) / m), lo, hi)
                osum = -256
            elif kind == "osum_max":
                wa = wb = _clamp(round(u * (64 - 127) / m), lo, hi)
                osum = 254
            else:                                                         # opposite: the difference of the two lists around an offset
                wa = int(rng.integers(u, 128 - u + 1))
                wb = -wa
                osum = 2 * 112
            osum = _clamp(round(osum), -256, 254)
            if kind in ("osum_min", "osum_max"):
                oa = ob = osum // 2
            else:
                oa = _clamp(osum // 2 + jit, -128, 127)
                ob = _clamp(osum - oa, -128, 127)
            _store(pic, pb, first, k, wa, oa, bd)
            _store(pic, pb, 1 - first, k, wb, ob, bd)
    return pic


def pb_kinds(pic, pb):
    """the corner kinds a PB's LUMA records show (read from the lists, not from how corner_weights dealt them)"""
    bdl, _ = _depths(pic)
    used = _lists(pb)
    recs = [pic.wts[int(pb["wt_idx"][l])] for l in used]
    u = 1 << (int(recs[0]["log2wd_luma"]) - max(2, 14 - bdl))
    ws = [int(r["w"][0]) for r in recs]
    os_ = [int(r["o"][0]) >> (bdl - 8) for r in recs]
    out = set()
    if u + 127 in ws:
        out.add("w_max")
    if u - 128 in ws and u != 128:                                        # (at denominator 7 that weight is 0: counted as such)
        out.add("w_min")
    if len(used) == 1:
        if ws[0] == 0:
            out.add("w_zero_alone")
        if os_[0] == -128:
            out.add("o_min")
        if os_[0] == 127:
            out.add("o_max")
    else:
        if sorted(w == 0 for w in ws) == [False, True]:
            out.add("w_zero_of_two")
        if sum(os_) == -256:
            out.add("osum_min")
        if sum(os_) == 254:
            out.add("osum_max")
        if ws[0] == -ws[1] != 0:
            out.add("opposite")
    return out


def _blocks(pic, pb, planes):
    """the PB's block of every plane, with that plane's maxv"""
    bdl, bdc = _depths(pic)
    sw, sh = _sub(pic)
    x, y, w, h = int(pb["x"]), int(pb["y"]), int(pb["w"]), int(pb["h"])
    out = [(planes[0][y:y + h, x:x + w], (1 << bdl) - 1)]
    for c in range(1, len(planes)):
        out.append((planes[c][y // sh:(y + h) // sh, x // sw:(x + w) // sw], (1 << bdc) - 1))
    return out


def weighted_census(pic, planes):
    """over the samples of the PBs with explicit weights, from decoded planes (inter prediction alone, or a picture without residuals) ->
    dict(pbs, planes=[dict(samples, unclipped (0 < v < maxv: a sample that lands on 0 or maxv without the clip counts as clipped), clean (PBs
    without a clipped sample))], classes={(lists, luma denominator): dict(pbs, samples, unclipped)} of luma, negative=dict(pbs (a negative
    weight in a list they use, any component), samples, unclipped (all planes)))"""
    bdl, _ = _depths(pic)
    idx = weighted_pbs(pic)
    out = dict(pbs=len(idx), planes=[dict(samples=0, unclipped=0, clean=0) for _ in planes], classes={}, negative=dict(pbs=0, samples=0, unclipped=0))
    for i in idx:
        pb = pic.pbs[i]
        used = _lists(pb)
        recs = [pic.wts[int(pb["wt_idx"][l])] for l in used]
        neg = any(int(r["w"][k]) < 0 for r in recs for k in range(len(planes)))
        out["negative"]["pbs"] += int(neg)
        for c, (a, maxv) in enumerate(_blocks(pic, pb, planes)):
            inside = int(((a > 0) & (a < maxv)).sum())
            e = out["planes"][c]
            e["samples"] += a.size
            e["unclipped"] += inside
            e["clean"] += int(inside == a.size)
            if neg:
                out["negative"]["samples"] += a.size
                out["negative"]["unclipped"] += inside
            if c == 0:
                cl = out["classes"].setdefault((len(used), int(recs[0]["log2wd_luma"]) - max(2, 14 - bdl)), dict(pbs=0, samples=0, unclipped=0))
                cl["pbs"] += 1
                cl["samples"] += a.size
                cl["unclipped"] += inside
    return out


def corner_census(pic, planes):
    """{kind: [PBs that show it (pb_kinds), of which GOOD]}: no sample of any plane clipped and the luma block not constant — for w_zero_alone,
    whose luma block is the constant o by the formula, not all samples of the PB's planes equal: its chroma carries a gain"""
    out = dict((k, [0, 0]) for k in CORNER_KINDS)
    for i in weighted_pbs(pic):
        pb = pic.pbs[i]
        blocks = _blocks(pic, pb, planes)
        clean = all(bool(((a > 0) & (a < maxv)).all()) for a, maxv in blocks)
        for kind in pb_kinds(pic, pb):
            varied = (blocks[0][0].min() != blocks[0][0].max()) if kind != "w_zero_alone" else any(a.min() != a.max() for a, _ in blocks[1:])
            out[kind][0] += 1
            out[kind][1] += int(clean and bool(varied))
    return out


# ---- the same two families for the write-back FUNCTIONS (test_oracle_vs_ref.py, slot_checks.py): one (w1, o1, w2, o2) per call, offsets in
# samples of depth bd; rng is a util.XorShift32 ----

FUNCTION_DIM = 2      # corner sets: intermediates of samples shifted right by 2, as the corner pictures' references


def _gain_scale(bd):
    """what a gain of 1 is worth: above 12 bits the intermediates keep 14 bits while log2WD still adds max(2, 14 - bd), a gain of 1/4 at 14
    bits and of 1/16 at 16"""
    return 2.0 ** (14 - bd - max(2, 14 - bd))


def inrange_sets(rng, bd, d):
    """three sets of denominator d: a positive gain of 0.5 .. 1.25, a negative one (down to -0.5; at d = 0 only -1 exists), one anywhere in
    the range of inrange_weights; the second list's weight ~ 2 - w1.  Offsets map mid-grey to mid-grey in either form"""
    u, sc = 1 << d, _gain_scale(bd)
    lo, hi = u - 128, u + 127
    out = []
    for k in range(3):
        if k == 0:
            w1 = rng.range((u + 1) // 2, 5 * u // 4)
        elif k == 1:
            w1 = rng.range(-max(1, u // 2), -1)
        else:
            w1 = rng.range(max(lo, -u), min(hi, 5 * u // 4))
        w1 = _clamp(w1, lo, hi)
        w2 = _clamp(2 * u - w1 + rng.range(-(u // 4), u // 4), lo, hi)
        o1 = _clamp(round(128 * (1 - sc * w1 / u)) + rng.range(-8, 8), -128, 127)
        # (the one-list form takes w1, o1 alone; the two-list form adds o2 so that o1 + o2 centres the pair)
        o2 = _clamp(round(256 * (1 - sc * (w1 + w2) / (2 * u))) - o1, -128, 127)
        out.append((w1, o1 << (bd - 8), w2, o2 << (bd - 8)))
    return out


def corner_sets(bd, d):
    """the ends of the legal ranges at denominator d (5..7), for intermediates dimmed by FUNCTION_DIM (expected content 32 of 256): each of
    CORNER_KINDS at least once over the one-list form (w1, o1) and the two-list form"""
    assert 5 <= d <= 7
    u, sc, m = 1 << d, _gain_scale(bd), 128 >> FUNCTION_DIM
    lo, hi = u - 128, u + 127

    def centre(gain, target=128):
        return _clamp(round(target - sc * gain * m), -128, 127)
    sets = [
        (hi, centre(hi / u), _clamp(2 * u - hi, lo, hi), centre(1) * 2 - centre(hi / u)),              # w_max | w_max with its complement
        (lo, centre(lo / u), _clamp(2 * u - lo, lo, hi), centre(1) * 2 - centre(lo / u)),              # w_min | w_min with its complement
        (0, 77, _clamp(2 * u, lo, hi), 2 * centre(_clamp(2 * u, lo, hi) / (2 * u)) - 77),              # w = 0 alone | as one of two
        (hi, -128, hi, -128),                                                                          # o_min | osum_min
        (lo, 127, lo, 127),                                                                            # o_max | osum_max
        (min(hi, 128 - u) if d < 7 else hi, 100, -(min(hi, 128 - u)) if d < 7 else lo, 100),           # opposite (d < 7) around an offset
    ]
    return [(w1, _clamp(o1, -128, 127) << (bd - 8), w2, _clamp(o2, -128, 127) << (bd - 8)) for (w1, o1, w2, o2) in sets]
