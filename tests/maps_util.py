"""Scenarios of the side-map tests (m355_picture_maps_async / _result / _order, m355_maps_unit), shared by the CPU tier (SIMT-interpreter build,
tests/test_maps_emu.py), the GPU tier (tests/test_gpu_maps.py) and the host-helper test (tests/test_maps_host.py), and the numpy restatement
their expected values come from.  The restatement PAINTS: every record that counts is written, as a slice assignment, into arrays on the 4x4 grid
of the picture, and a unit reads the array at its top-left luma position.  It shares no code with csrc/map_element.h.  Every comparison is exact.

Before a synthetic picture is used its PRECONDITION is asserted: each of {CU}, {TU} and {PB + luma IB} covers every 4x4 unit of the picture
exactly once — so a wrong restatement cannot hide behind overlapping records, whose winner the definition leaves open."""
import ctypes
import json
import os

import numpy as np
import pytest

from hash_util import CRC
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from libde265_amd import capi, synth, worklist

BUSY, INVALID = 6, 3                # M355_ERR_BUSY, M355_ERR_INVALID
SLOTS = capi.MAPS_REQUESTS
ALL = tuple(range(capi.N_MAPS))
UNITS = (2, 3, 4, 5, 6)
NONE_CU, NONE_QP, NONE_TU, NONE_INTRA = 0xFFFFFFFF, -128, 0, 255

# scenario 1: the smallest pictures at which the kernels can still go wrong — CTBs and units of 64 that hang over both edges (72x40 under a 64x64
# CTB; clipped_picture() adds RECORDS that do), small CTBs with many intra units, an EMPTY prediction-block list, and tiles + slices + PCM + AMP
# partitions (12x16, 16x4, 4x16 PBs)
GEOMETRIES = {
    "72x40_ctb64": dict(width=72, height=40, log2_ctb=6),
    "200x120_ctb16": dict(width=200, height=120, log2_ctb=4, intra_pct=40),
    "136x72_ctb32_intra": dict(width=136, height=72, log2_ctb=5, intra_pct=100, n_refs=0),
    "416x240_tiles_slices_pcm": dict(width=416, height=240, tile_cols=2, tile_rows=2, n_slices=3, features=synth.SYN_PCM, seed=7),
}
_PICS = {}


# ---- the restatement ----
def _dims(pic):
    pp = pic.pp[0]
    return int(pp["width"]), int(pp["height"])


def _cells(lo, n, limit):
    """points of the 4-sample grid inside lo .. lo + n, cut to the picture: a slice"""
    return slice(-(-lo // 4), min(-(-(lo + n) // 4), limit))


def counted(pic):
    """per list the boolean array "this record counts" (the geometry clauses, restated), in the order cu, tu, pb, ib"""
    pp = pic.pp[0]
    W, H = _dims(pic)
    cf = int(pp["chroma_format_idc"])
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    cu, tu, pb, ib = pic.cus, pic.tus, pic.pbs, pic.ibs
    cu_ok = (cu["log2_size"] >= pp["log2_min_cb_size"]) & (cu["log2_size"] <= pp["log2_ctb_size"]) & (cu["x"] < W) & (cu["y"] < H) & \
            (cu["pred_mode"] <= 2) & (cu["part_mode"] <= 7)
    tu_ok = (tu["log2_size"] >= 2) & (tu["log2_size"] <= 6) & (tu["x"] < W) & (tu["y"] < H)
    pw, ph = pb["w"].astype(np.int64), pb["h"].astype(np.int64)
    pb_ok = (pw >= 4) & (ph >= 4) & (pw <= 64) & (ph <= 64) & (pw % 4 == 0) & (ph % 4 == 0) & (pb["x"] + pw <= W) & (pb["y"] + ph <= H)
    n = np.int64(1) << np.minimum(ib["log2_size"].astype(np.int64), 16)
    cw = np.where(ib["cidx"] > 0, W // sw, W)
    ch = np.where(ib["cidx"] > 0, H // sh, H)
    ib_ok = (ib["log2_size"] >= 2) & (ib["log2_size"] <= 5) & (ib["cidx"] <= 2) & (ib["mode"] <= 34) & (ib["x"] + n <= cw) & (ib["y"] + n <= ch)
    return cu_ok, tu_ok, pb_ok, ib_ok


def paint(pic):
    """-> dict of (h4, w4) arrays on the picture's 4x4 grid: the index of the record painted last (-1: none) for cu / tu / pb / ib (the luma intra
    blocks that are not PCM), and how many records were painted per cell for cu / tu / pb + every luma intra block (the precondition)"""
    W, H = _dims(pic)
    w4, h4 = -(-W // 4), -(-H // 4)
    cu_ok, tu_ok, pb_ok, ib_ok = counted(pic)
    out = {k: np.full((h4, w4), -1, np.int64) for k in ("cu", "tu", "pb", "ib")}
    cnt = {k: np.zeros((h4, w4), np.int64) for k in ("cu", "tu", "pred")}
    for i in np.flatnonzero(cu_ok):
        r = pic.cus[i]
        s = (_cells(int(r["y"]), 1 << int(r["log2_size"]), h4), _cells(int(r["x"]), 1 << int(r["log2_size"]), w4))
        out["cu"][s] = i; cnt["cu"][s] += 1
    for i in np.flatnonzero(tu_ok):
        r = pic.tus[i]
        s = (_cells(int(r["y"]), 1 << int(r["log2_size"]), h4), _cells(int(r["x"]), 1 << int(r["log2_size"]), w4))
        out["tu"][s] = i; cnt["tu"][s] += 1
    for i in np.flatnonzero(pb_ok):
        r = pic.pbs[i]
        s = (_cells(int(r["y"]), int(r["h"]), h4), _cells(int(r["x"]), int(r["w"]), w4))
        out["pb"][s] = i; cnt["pred"][s] += 1
    for i in np.flatnonzero(ib_ok & (pic.ibs["cidx"] == 0)):
        r = pic.ibs[i]
        s = (_cells(int(r["y"]), 1 << int(r["log2_size"]), h4), _cells(int(r["x"]), 1 << int(r["log2_size"]), w4))
        cnt["pred"][s] += 1
        if not int(r["flags"]) & worklist.IBF_PCM:
            out["ib"][s] = i
    out["count"] = cnt
    return out


def assert_precondition(pic, what=""):
    c = paint(pic)["count"]
    for k in ("cu", "tu", "pred"):
        assert (c[k] == 1).all(), "%s: the %s records do not cover every 4x4 unit exactly once (counts %d..%d)" % (what, k, c[k].min(), c[k].max())


def expected(pic, log2_unit, maps=ALL, painted=None):
    """what a request on these lists delivers -> ({map index: array}, info dict)"""
    W, H = _dims(pic)
    U, pp = 1 << log2_unit, pic.pp[0]
    uw, uh = -(-W // U), -(-H // U)
    p = painted if painted is not None else paint(pic)
    st = U // 4
    at = {k: p[k][::st, ::st] for k in ("cu", "tu", "pb", "ib")}
    assert at["cu"].shape == (uh, uw)
    out = {}
    cu_i, tu_i, pb_i, ib_i = at["cu"], at["tu"], at["pb"], at["ib"]
    cus, tus, pbs, ibs = pic.cus, pic.tus, pic.pbs, pic.ibs
    has_cu, has_pb = cu_i >= 0, pb_i >= 0
    cu_r = cus[np.maximum(cu_i, 0)] if len(cus) else np.zeros(cu_i.shape, worklist.CU)
    pb_r = pbs[np.maximum(pb_i, 0)] if len(pbs) else np.zeros(pb_i.shape, worklist.PB)
    cu_v = np.where(has_cu, cu_r["pred_mode"].astype(np.uint32) | (cu_r["part_mode"].astype(np.uint32) << 8) | (cu_r["log2_size"].astype(np.uint32) << 16) |
                    (cu_r["flags"].astype(np.uint32) << 24), np.uint32(NONE_CU)).astype(np.uint32)
    qp_v = np.where(has_cu, cu_r["qp_y"], np.int8(NONE_QP)).astype(np.int8)
    if capi.MAP_CU in maps:
        out[capi.MAP_CU] = cu_v
    if capi.MAP_QP in maps:
        out[capi.MAP_QP] = qp_v
    if capi.MAP_TU in maps:
        tu_r = tus[np.maximum(tu_i, 0)] if len(tus) else np.zeros(tu_i.shape, worklist.TU)
        out[capi.MAP_TU] = np.where(tu_i >= 0, tu_r["log2_size"] | np.where(tu_r["flags"] & worklist.TUF_NONZERO_COEFF, 0x80, 0), NONE_TU).astype(np.uint8)
    if capi.MAP_INTRA in maps:
        ib_r = ibs[np.maximum(ib_i, 0)] if len(ibs) else np.zeros(ib_i.shape, worklist.IB)
        out[capi.MAP_INTRA] = np.where(ib_i >= 0, ib_r["mode"], NONE_INTRA).astype(np.uint8)
    fl = pb_r["flags"]
    if capi.MAP_MV in maps:
        mv = np.zeros((uh, uw, 4), np.int16)
        for l in range(2):
            on = has_pb & ((fl & (worklist.PBF_PRED_L0 << l)) != 0)
            for k in range(2):
                mv[:, :, 2 * l + k] = np.where(on, pb_r["mv"][..., l, k], 0)
        out[capi.MAP_MV] = mv
    ref = np.zeros((uh, uw, 4), np.uint8)
    for l in range(2):
        ref[:, :, l] = np.where(has_pb & ((fl & (worklist.PBF_PRED_L0 << l)) != 0), pb_r["ref_slot"][..., l].astype(np.uint8), 0xFF)
    ref[:, :, 2] = np.where(has_pb, fl, 0)
    if capi.MAP_REF in maps:
        out[capi.MAP_REF] = ref
    if capi.MAP_SLICE in maps:
        lc = int(pp["log2_ctb_size"])
        ctb_w = -(-W // (1 << lc))
        ys, xs = np.meshgrid(np.arange(uh) * U, np.arange(uw) * U, indexing="ij")
        out[capi.MAP_SLICE] = pic.ctbs["slice_idx"][(ys >> lc) * ctb_w + (xs >> lc)].astype(np.uint16)
    info = dict(units_w=uw, units_h=uh, covered=0, n_intra=0, n_inter=0, n_skip=0, qp_sum=0, qp_min=127, qp_max=-128, n_bipred=0, skipped=[0, 0, 0, 0])
    if capi.MAP_CU in maps:
        pm = cu_r["pred_mode"][has_cu]
        info.update(n_intra=int((pm == 0).sum()), n_inter=int((pm == 1).sum()), n_skip=int((pm == 2).sum()), covered=int(has_cu.sum()))
    if capi.MAP_QP in maps and has_cu.any():
        q = qp_v[has_cu].astype(np.int64)
        info.update(qp_sum=int(q.sum()), qp_min=int(q.min()), qp_max=int(q.max()))
    if capi.MAP_REF in maps:
        info["n_bipred"] = int((has_pb & ((fl & 3) == 3)).sum())
    ok = counted(pic)
    read = (capi.MAP_CU in maps or capi.MAP_QP in maps, capi.MAP_TU in maps, capi.MAP_MV in maps or capi.MAP_REF in maps, capi.MAP_INTRA in maps)
    info["skipped"] = [int((~o).sum()) if r else 0 for o, r in zip(ok, read)]
    return out, info


def assert_maps(got, want, what=""):
    """got: (maps, info, guards_intact) of Context.picture_maps_result; want: expected()"""
    maps, info, intact = got
    wmaps, winfo = want
    assert sorted(maps) == sorted(wmaps), what
    for m in sorted(wmaps):
        g, w = maps[m], wmaps[m]
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: map %s is %s %s, expected %s %s" % (what, capi.MAP_NAMES[m], g.shape, g.dtype, w.shape, w.dtype)
        if not np.array_equal(g, w):
            d = np.argwhere(g != w)
            raise AssertionError("%s: map %s: %d elements differ, first at %s: got %r, expected %r" % (what, capi.MAP_NAMES[m], len(d), tuple(d[0]), g[tuple(d[0])], w[tuple(d[0])]))
    assert info == winfo, "%s: summary %r, expected %r" % (what, info, winfo)
    assert intact, "%s: bytes outside the rows were written" % what


# ---- pictures ----
def synthetic(name):
    """a picture of scenario 1 (made once, never changed; reference slots 0 and 1 named, no frames behind them) with its painting"""
    if name not in _PICS:
        pic = synth.picture(**GEOMETRIES[name])
        n_refs = pic.meta["cfg"]["n_refs"]
        pic.ref_frames = [i if i < n_refs else -1 for i in range(worklist.MAX_REF_FRAMES)]
        pic.dst_frame = -1
        assert_precondition(pic, name)
        _PICS[name] = (pic, paint(pic))
    return _PICS[name]


def assert_geometries_reach_their_cases():
    """what the issue promises of the four geometries: an empty PB list, AMP partitions with 12x16 / 16x4 / 4x16 PBs, PCM blocks, several slices"""
    assert len(synthetic("136x72_ctb32_intra")[0].pbs) == 0
    pic = synthetic("416x240_tiles_slices_pcm")[0]
    sizes = set(zip(pic.pbs["w"].tolist(), pic.pbs["h"].tolist()))
    assert {(12, 16), (16, 4), (4, 16)} <= sizes, sorted(sizes)
    assert set(pic.cus["part_mode"].tolist()) & {4, 5, 6, 7}
    assert int(((pic.ibs["flags"] & worklist.IBF_PCM) != 0).sum()) == 18 and int(((pic.ibs["flags"] & worklist.IBF_PCM) != 0)[pic.ibs["cidx"] == 0].sum()) == 6
    assert len(set(pic.ctbs["slice_idx"].tolist())) >= 2            # (the generator starts slices at tile boundaries: n_slices=3 gives two here)
    # (the generator, like an encoder, splits coding units at the picture's edges: in 72x40 the CTBs and the units of 64 hang over both edges, no
    # record does — clipped_picture() below has the records that do)
    cu = synthetic("72x40_ctb64")[0].cus
    assert ((cu["x"] + (1 << cu["log2_size"].astype(np.int64)) <= 72) & (cu["y"] + (1 << cu["log2_size"].astype(np.int64)) <= 40)).all()


def clipped_picture():
    """72x40 under a 64x64 CTB with RECORDS that hang over the edges: two 64x64 coding units and six 32x32 transform units, each cut by the right
    edge, the bottom edge or both (the record checks ask for a position inside the picture, not for an end inside it)"""
    pic = synthetic("72x40_ctb64")[0].copy()
    cus = np.zeros(2, worklist.CU)
    cus["x"], cus["y"], cus["log2_size"], cus["pred_mode"], cus["qp_y"], cus["flags"] = [0, 64], 0, 6, [1, 2], [-3, 44], [0, 2]
    tus = np.zeros(6, worklist.TU)
    tus["x"], tus["y"], tus["log2_size"], tus["flags"] = [0, 32, 0, 32, 64, 64], [0, 0, 32, 32, 0, 32], 5, [1, 0, 0, 1, 1, 0]
    pic.cus, pic.tus = cus, tus
    assert_precondition(pic, "clipped records")
    return pic


def sampling_picture():
    """scenario 2: 16x16, one CTB, four 8x8 CUs — 8x4 PBs, 4x8 PBs, and twice four 4x4 intra blocks — with a value of its own in every record, so
    that the top-left 4x4 of each 8x8 and of the 16x16 unit differs from the rest of that unit"""
    pic = synth.picture(width=16, height=16, log2_ctb=4, n_refs=2, seed=3)
    pic.ref_frames = [0, 1] + [-1] * (worklist.MAX_REF_FRAMES - 2)
    pic.dst_frame = -1
    cus = np.zeros(4, worklist.CU)
    cus["x"], cus["y"], cus["log2_size"] = [0, 8, 0, 8], [0, 0, 8, 8], 3
    cus["pred_mode"], cus["part_mode"], cus["qp_y"] = [1, 2, 0, 0], [1, 2, 3, 3], [-7, 22, 30, 51]
    pbs = np.zeros(4, worklist.PB)
    pbs["x"], pbs["y"], pbs["w"], pbs["h"] = [0, 0, 8, 12], [0, 4, 0, 0], [8, 8, 4, 4], [4, 4, 8, 8]
    pbs["flags"] = [worklist.PBF_PRED_L0 | worklist.PBF_MC_L0, worklist.PBF_PRED_L1 | worklist.PBF_MC_L1,
                    worklist.PBF_PRED_L0 | worklist.PBF_PRED_L1 | worklist.PBF_MC_L0 | worklist.PBF_MC_L1, worklist.PBF_PRED_L0 | worklist.PBF_MC_L0]
    pbs["ref_slot"] = [[0, 1], [1, 0], [1, 0], [1, -1]]
    pbs["mv"] = [[[3, -5], [111, 112]], [[113, 114], [-32768, 32767]], [[7, 9], [-11, 13]], [[-1, 1], [115, 116]]]
    ibs = np.zeros(8, worklist.IB)
    ibs["x"], ibs["y"] = [0, 4, 0, 4, 8, 12, 8, 12], [8, 8, 12, 12, 8, 8, 12, 12]
    ibs["log2_size"], ibs["mode"] = 2, [0, 1, 10, 26, 34, 2, 18, 33]
    tus = np.zeros(13, worklist.TU)                     # an 8x8 leaf over CU 1, 4x4 leaves elsewhere, the coded flag on every other one
    tus["x"] = [0, 4, 0, 4, 8, 0, 4, 0, 4, 8, 12, 8, 12]
    tus["y"] = [0, 0, 4, 4, 0, 8, 8, 12, 12, 8, 8, 12, 12]
    tus["log2_size"] = [2, 2, 2, 2, 3, 2, 2, 2, 2, 2, 2, 2, 2]
    tus["flags"] = [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0]
    pic.cus, pic.tus, pic.pbs, pic.ibs = cus, tus, pbs, ibs
    pic.wts = np.zeros(0, worklist.WT)
    pic.rbs, pic.rb_count, pic.coeffs, pic.pcm, pic.res_len = np.zeros(0, worklist.RB), [0, 0, 0, 0], np.zeros(0, "<u4"), np.zeros(0, "<u2"), 0
    pic.ctbs["ib_start"], pic.ctbs["ib_count"] = 0, len(ibs)
    assert_precondition(pic, "sampling picture")
    return pic


def without_one_cu(pic, which):
    """scenario 4: a copy of `pic` without CU `which` and without the TUs, PBs and intra blocks (of every component) inside it -> (copy, its cells)"""
    W, H = _dims(pic)
    pp = pic.pp[0]
    cf = int(pp["chroma_format_idc"])
    sw, sh = (2 if cf in (1, 2) else 1), (2 if cf == 1 else 1)
    c = pic.cus[which]
    x0, y0, n = int(c["x"]), int(c["y"]), 1 << int(c["log2_size"])

    def inside(x, y, sx=1, sy=1):
        return (x * sx >= x0) & (x * sx < x0 + n) & (y * sy >= y0) & (y * sy < y0 + n)

    out = pic.copy()
    out.cus = np.delete(pic.cus, which)
    out.tus = pic.tus[~inside(pic.tus["x"].astype(np.int64), pic.tus["y"].astype(np.int64))]
    out.pbs = pic.pbs[~inside(pic.pbs["x"].astype(np.int64), pic.pbs["y"].astype(np.int64))]
    ib = pic.ibs
    drop = inside(ib["x"].astype(np.int64), ib["y"].astype(np.int64), np.where(ib["cidx"] > 0, sw, 1), np.where(ib["cidx"] > 0, sh, 1))
    owner = np.repeat(np.arange(len(pic.ctbs)), pic.ctbs["ib_count"].astype(np.int64))          # (each CTB's blocks are one run, in CTB order)
    assert np.array_equal(pic.ctbs["ib_start"], np.cumsum(pic.ctbs["ib_count"]) - pic.ctbs["ib_count"])
    out.ibs = ib[~drop]
    out.ctbs = pic.ctbs.copy()
    out.ctbs["ib_count"] = np.bincount(owner[~drop], minlength=len(pic.ctbs)).astype(np.uint32)
    out.ctbs["ib_start"] = (np.cumsum(out.ctbs["ib_count"]) - out.ctbs["ib_count"]).astype(np.uint32)
    w4, h4 = -(-W // 4), -(-H // 4)
    return out, (_cells(y0, n, h4), _cells(x0, n, w4))


# ---- running requests ----
def run(ctx, handle, pic, log2_unit, maps=ALL, what="", painted=None, **kw):
    want = expected(pic, log2_unit, maps, painted)
    got = ctx.picture_maps_result(ctx.picture_maps_async(handle, log2_unit, maps=maps, **kw))
    assert_maps(got, want, "%s unit %d maps %s %s" % (what, 1 << log2_unit, maps, kw or ""))
    return want


# 1 (and 10: the summary is part of every comparison)
def check_geometry(ctx, name, log2_unit):
    """a picture uploaded and never decoded, every map"""
    pic, painted = synthetic(name)
    h = ctx.upload(pic)
    try:
        run(ctx, h, pic, log2_unit, what=name, painted=painted)
    finally:
        ctx.release(h)


def check_clipped(ctx):
    pic = clipped_picture()
    h = ctx.upload(pic)
    try:
        for lu in UNITS:
            run(ctx, h, pic, lu, what="records over the edges")
    finally:
        ctx.release(h)


# 2
def check_sampling(ctx):
    pic = sampling_picture()
    h = ctx.upload(pic)
    try:
        seen = []
        for lu in (2, 3, 4):
            maps, _ = run(ctx, h, pic, lu, what="sampling")
            seen.append(maps)
        # the restatement itself: the coarser grids are the finer one's top-left values, and those differ from the rest of their unit
        fine = seen[0]
        for m in (capi.MAP_QP, capi.MAP_INTRA, capi.MAP_MV, capi.MAP_TU):
            assert np.array_equal(seen[1][m], fine[m][::2, ::2]) and np.array_equal(seen[2][m], fine[m][::4, ::4])
        assert fine[capi.MAP_MV][0, 0].tolist() == [3, -5, 0, 0] and fine[capi.MAP_MV][1, 0].tolist() == [0, 0, -32768, 32767]
        assert fine[capi.MAP_MV][0, 2].tolist() == [7, 9, -11, 13] and fine[capi.MAP_MV][0, 3].tolist() == [-1, 1, 0, 0]
        assert fine[capi.MAP_INTRA].tolist() == [[255] * 4, [255] * 4, [0, 1, 34, 2], [10, 26, 18, 33]]
        assert fine[capi.MAP_TU].tolist() == [[0x82, 2, 3, 3], [2, 0x82, 3, 3], [0x82, 2, 2, 0x82], [0x82, 2, 0x82, 2]]
        assert fine[capi.MAP_REF][0, 3].tolist() == [1, 255, 5, 0] and fine[capi.MAP_REF][1, 1].tolist() == [255, 0, 10, 0]
        assert seen[2][capi.MAP_QP].tolist() == [[-7]] and seen[1][capi.MAP_QP].tolist() == [[-7, 22], [30, 51]]
    finally:
        ctx.release(h)


# 3
def check_destinations(ctx):
    """the pitch 20 bytes above the row (24 for MAP_MV, whose pitch is a multiple of 8), pointers 1 and 3 elements off a 256-byte boundary, pinned host
    memory, each map alone and all together; guard bytes behind every row and guard rows in front and behind are part of every comparison"""
    pic, painted = synthetic("200x120_ctb16")
    h = ctx.upload(pic)
    try:
        for lu in (2, 4):
            for mis in (0, 1, 3):
                run(ctx, h, pic, lu, what="destinations", painted=painted, misalign=mis)
            run(ctx, h, pic, lu, what="destinations, host memory", painted=painted, host=True, misalign=1)
            run(ctx, h, pic, lu, what="destinations, tight pitch", painted=painted, pad=0)
        for m in ALL:
            for mis in (0, 1):
                run(ctx, h, pic, 2, maps=(m,), what="one map", painted=painted, misalign=mis)
    finally:
        ctx.release(h)


# 4 (and 10)
def check_uncovered(ctx):
    pic, painted = synthetic("200x120_ctb16")
    inter = np.flatnonzero(pic.cus["pred_mode"] != 0)
    intra = np.flatnonzero(pic.cus["pred_mode"] == 0)
    for which in (int(inter[len(inter) // 2]), int(intra[len(intra) // 2])):
        cut, cells = without_one_cu(pic, which)
        h = ctx.upload(cut)
        try:
            for lu in (2, 3):
                (maps, info), (maps0, info0) = run(ctx, h, cut, lu, what="one CU removed"), expected(pic, lu, painted=painted)
                st = (1 << lu) // 4
                hole = np.zeros(painted["cu"].shape, bool)
                hole[cells] = True
                hole = hole[::st, ::st]
                assert hole.any() or lu > 2
                assert (maps[capi.MAP_CU][hole] == NONE_CU).all() and (maps[capi.MAP_QP][hole] == NONE_QP).all() and (maps[capi.MAP_TU][hole] == NONE_TU).all()
                assert (maps[capi.MAP_INTRA][hole] == NONE_INTRA).all() and (maps[capi.MAP_MV][hole] == 0).all()
                assert (maps[capi.MAP_REF][hole] == np.array([255, 255, 0, 0], np.uint8)).all()
                for m in ALL:
                    assert np.array_equal(maps[m][~hole], maps0[m][~hole]), "map %s outside the hole" % capi.MAP_NAMES[m]
                assert info["covered"] == info0["covered"] - int(hole.sum())
        finally:
            ctx.release(h)


# 5
def skipped_pictures():
    """-> [(what, picture, which list's record is bad)]: 72x40 under a 64x64 CTB, half intra, with ONE record given a position outside the picture
    (an intra block's must stay inside its CTB, which hangs over the picture's edge: the host's schedules index by it) or a PB a width of 6"""
    base = synth.picture(width=72, height=40, log2_ctb=6, intra_pct=50, seed=5)
    base.ref_frames = [0, 1] + [-1] * (worklist.MAX_REF_FRAMES - 2)
    base.dst_frame = -1
    assert_precondition(base, "skipped records")
    out = []
    for what, lst, field, pick, value in (("cu beyond the right edge", "cus", "x", None, 72), ("tu below the picture", "tus", "y", None, 40),
                                          ("pb 6 wide", "pbs", "w", None, 6), ("pb beyond the bottom edge", "pbs", "y", None, 40),
                                          ("luma intra block beyond the right edge", "ibs", "x", "luma_right", 72)):
        pic = base.copy()
        arr = getattr(pic, lst).copy()
        if pick == "luma_right":
            cand = np.flatnonzero((arr["cidx"] == 0) & (arr["x"] >= 64) & ((arr["flags"] & worklist.IBF_PCM) == 0))
            assert len(cand), "the picture needs a luma intra block in its second CTB"
            i = int(cand[0])
        else:
            i = len(arr) // 2
        arr[field][i] = value
        setattr(pic, lst, arr)
        out.append((what, pic, ("cus", "tus", "pbs", "ibs").index(lst)))
    return out


def check_skipped(ctx):
    for what, pic, lst in skipped_pictures():
        with pytest.raises(capi.M355Error) as e:                    # the copying upload checks every record on the host
            ctx.upload(pic)
        assert e.value.code == INVALID, what
        h = ctx.upload_in_place(pic)
        try:
            for lu in (2, 3):
                _, info = run(ctx, h, pic, lu, what=what)
                assert info["skipped"][lst] == 1 and sum(info["skipped"]) == 1, what
        finally:
            ctx.release(h)


# 6
def check_replace_hazard(ctx):
    """request, then m355_picture_replace with other lists at once: the result is the earlier lists'"""
    (a, pa), (b, pb) = synthetic("200x120_ctb16"), synthetic("136x72_ctb32_intra")
    h = ctx.upload(a)
    try:
        want_a = expected(a, 2, painted=pa)
        for k in range(3):
            tk = ctx.picture_maps_async(h, 2)
            ctx.replace(h, b)
            tk_b = ctx.picture_maps_async(h, 3)
            ctx.replace(h, a)
            assert_maps(ctx.picture_maps_result(tk), want_a, "the lists replaced behind the request, round %d" % k)
            assert_maps(ctx.picture_maps_result(tk_b), expected(b, 3, painted=pb), "the lists that replaced them, round %d" % k)
    finally:
        ctx.release(h)


def check_submit_ring(lib, oracle, depth):
    """six m355_submit_picture of different pictures, each followed by a request on M355_PICTURE_LAST, nothing waited for in between (the ring of
    three arenas wraps twice): every result is its own picture's, and the decodes are the oracle's"""
    o = Oracle(oracle)
    cases = [make_case(width=200, height=120, log2_ctb=4, intra_pct=20 + 10 * k, seed=40 + k) for k in range(6)]
    want_planes = [oracle_decode(o, pic, refs) for pic, refs in cases]
    ctx = capi.Context(lib, 0)
    try:
        pp = cases[0][0].pp[0]
        refs = []
        for _, planes_of in cases:
            refs.append([ctx.frame_create_for(pp) for _ in planes_of])
            for f, planes in zip(refs[-1], planes_of):
                ctx.frame_upload(f, planes)
        dsts = [ctx.frame_create_for(pp) for _ in cases]
        ctx.set_pipeline_depth(depth)
        with pytest.raises(capi.M355Error) as e:                    # (M355_PICTURE_LAST before any submit)
            ctx._pic_size[capi.PICTURE_LAST] = (200, 120)
            ctx.picture_maps_async(capi.PICTURE_LAST, 2)
        assert e.value.code == INVALID
        tickets = []
        for k, (pic, _) in enumerate(cases):
            pic.dst_frame = dsts[k]
            pic.ref_frames = [refs[k][i] if i < len(refs[k]) else -1 for i in range(worklist.MAX_REF_FRAMES)]
            assert_precondition(pic, "picture %d" % k)
            ctx.submit(pic)
            tickets.append(ctx.picture_maps_async(capi.PICTURE_LAST, 2 + k % 3))
        for k, (pic, _) in enumerate(cases):
            assert_maps(ctx.picture_maps_result(tickets[k]), expected(pic, 2 + k % 3), "picture %d of six, depth %d" % (k, depth))
        ctx.wait()
        for k in range(6):
            assert_planes_equal(ctx.frame_download(dsts[k]), want_planes[k], "picture %d" % k)
    finally:
        ctx.close()


# 7
def check_concurrency(lib):
    """16 requests before any is collected, collected in reverse; the 17th is refused; a collected slot is free again"""
    ctx = capi.Context(lib, 0)
    try:
        names = list(GEOMETRIES)
        hs = {n: ctx.upload(synthetic(n)[0]) for n in names}
        args = [(names[i % 4], 2 + i % 5, ALL if i % 3 else (capi.MAP_MV, capi.MAP_REF)) for i in range(SLOTS)]
        want = [expected(synthetic(n)[0], lu, maps, synthetic(n)[1]) for n, lu, maps in args]
        tickets = [ctx.picture_maps_async(hs[n], lu, maps=maps) for n, lu, maps in args]
        assert tickets == list(range(1, SLOTS + 1)), "tickets count 1, 2, ... per context"
        with pytest.raises(capi.M355Error) as e:
            ctx.picture_maps_async(hs[names[0]], 2)
        assert e.value.code == BUSY
        assert_maps(ctx.picture_maps_result(tickets[-1]), want[-1], "the last request")
        extra = ctx.picture_maps_async(hs[args[3][0]], args[3][1], maps=args[3][2])     # the refused call took no ticket and enqueued nothing
        assert extra == SLOTS + 1
        assert_maps(ctx.picture_maps_result(extra), want[3], "the slot collected first, reused")
        for i in reversed(range(SLOTS - 1)):
            assert_maps(ctx.picture_maps_result(tickets[i]), want[i], "request %d" % i)
    finally:
        ctx.close()


def check_nonblocking(lib):
    ctx = capi.Context(lib, 0)
    try:
        pic, painted = synthetic("200x120_ctb16")
        h = ctx.upload(pic)
        want = expected(pic, 2, painted=painted)
        for k in range(3):
            tk = ctx.picture_maps_async(h, 2)
            assert tk == k + 1
            got = ctx.picture_maps_result(tk, block=False)
            while got is None:                                      # BUSY: nothing was waited for, the request stays
                got = ctx.picture_maps_result(tk, block=False)
            assert_maps(got, want, "non-blocking collection")
            for bad in (tk, tk + 1000, 0):                          # collected / unknown
                with pytest.raises(capi.M355Error) as e:
                    ctx.picture_maps_result(bad, block=False)
                assert e.value.code == INVALID
        tk = ctx.picture_maps_async(h, 2)                           # m355_wait completes a request and does not collect it
        ctx.wait()
        assert_maps(ctx.picture_maps_result(tk, block=False), want, "collected behind m355_wait")
        tk = ctx.picture_maps_async(h, 3)                           # the picture released with a request pending: the release waits for it
        bufs = ctx._maps_reqs[tk]
        ctx.release(h)
        assert_maps(ctx.picture_maps_result(tk), expected(pic, 3, painted=painted), "collected behind the picture's release")
        assert bufs
    finally:
        ctx.close()
    # a context destroyed with requests pending
    ctx = capi.Context(lib, 0)
    h = ctx.upload(pic)
    for lu in (2, 3, 4):
        ctx.picture_maps_async(h, lu)
    ctx.close()


def check_slot_reuse(ctx, rounds=40):
    """one slot, request after request on pictures and map sets that alternate: a device record not left zero shows in the next summary (counts added
    up, a stale smaller minimum or larger maximum, skip counts that stay)"""
    bad = skipped_pictures()[0][1]
    hb = ctx.upload_in_place(bad)
    names = list(GEOMETRIES)
    hs = {n: ctx.upload(synthetic(n)[0]) for n in names}
    try:
        for k in range(rounds):
            maps = (ALL, (capi.MAP_QP,), (capi.MAP_REF, capi.MAP_SLICE), (capi.MAP_CU, capi.MAP_TU))[k % 4]
            if k % 5 == 4:
                run(ctx, hb, bad, 2, maps=ALL, what="round %d" % k)
            else:
                n = names[k % 3]
                run(ctx, hs[n], synthetic(n)[0], 2 + k % 2, maps=maps, what="round %d" % k, painted=synthetic(n)[1])
    finally:
        for h in list(hs.values()) + [hb]:
            ctx.release(h)


def check_order(ctx, stream, read):
    """m355_picture_maps_order onto `stream`, then read(pointer, nbytes) -> uint8 array, a device read ON that stream with nothing else waited for"""
    pic, painted = synthetic("416x240_tiles_slices_pcm")
    h = ctx.upload(pic)
    try:
        want, _ = expected(pic, 2, (capi.MAP_MV,), painted)
        tk = ctx.picture_maps_async(h, 2, maps=(capi.MAP_MV,), pad=0)
        ctx.picture_maps_order(tk, stream)
        p, ofs, pitch, rows, row, nbytes = ctx._maps_reqs[tk][0][capi.MAP_MV]
        raw = read(p + ofs, rows * pitch)
        got = raw.view("<i2").reshape(want[capi.MAP_MV].shape)
        assert np.array_equal(got, want[capi.MAP_MV]), "read on the consumer's stream behind m355_picture_maps_order"
        with pytest.raises(capi.M355Error) as e:
            ctx.picture_maps_order(tk + 99, stream)
        assert e.value.code == INVALID
        assert_maps(ctx.picture_maps_result(tk), (want, expected(pic, 2, (capi.MAP_MV,), painted)[1]), "the request stays to be collected")
    finally:
        ctx.release(h)


# 8
def rejections():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maps_rejections.json")) as f:
        return json.load(f)


def check_rejection(lib, case):
    """one refused call of tests/golden/maps_rejections.json: M355_ERR_INVALID, no byte of any destination written, and no slot taken — sixteen
    requests succeed behind it, with consecutive tickets"""
    pic, painted = synthetic("72x40_ctb64")
    W, H = _dims(pic)
    ctx = capi.Context(lib, 0)
    try:
        if case.get("sharded"):
            h = 0                                                   # (a sharded context refuses before it looks at the handle's lists)
            ctx.shard_set(0, 2)
        else:
            h = ctx.upload(pic)
        lu = case.get("log2_unit", 2)
        g = min(max(lu, 2), 6)
        uw, uh = -(-W // (1 << g)), -(-H // (1 << g))
        desc = capi.MapsDesc(log2_unit=lu, reserved=case.get("reserved", 0))
        bufs = {}
        for m in case.get("maps", list(ALL)):
            es = capi.MAP_ELEM_BYTES[m]
            pitch = uw * es + 8 + case.get("pitch_delta", {}).get(str(m), 0)
            nbytes = (uh + 2) * (uw * es + 16) + 64
            bufs[m] = (ctx.device_alloc(nbytes), nbytes)
            desc.dst[m] = bufs[m][0] + 16 + case.get("pointer_delta", {}).get(str(m), 0)
            desc.pitch[m] = pitch
        tk = ctypes.c_ulonglong(0)
        handle = {"resident": h, "beyond": h + 99, "negative": -2, "last": capi.PICTURE_LAST}[case.get("handle", "resident")]
        rc = lib.lib.m355_picture_maps_async(ctx.h, handle, None if case.get("null_desc") else ctypes.byref(desc), None if case.get("null_ticket") else ctypes.byref(tk))
        assert rc == INVALID, "%s: returned %d" % (case["what"], rc)
        for m, (p, nbytes) in bufs.items():
            assert (ctx.device_read(p, nbytes) == capi.DEVICE_FILL).all(), "%s: a byte of map %d was written" % (case["what"], m)
            ctx.device_free(p)
        if case.get("sharded"):
            return
        tickets = [ctx.picture_maps_async(h, 2 + k % 5, maps=(capi.MAP_CU, capi.MAP_SLICE)) for k in range(SLOTS)]
        assert tickets == list(range(1, SLOTS + 1)), "%s: a slot or a ticket was taken" % case["what"]
        for k, t in enumerate(tickets):
            assert_maps(ctx.picture_maps_result(t), expected(pic, 2 + k % 5, (capi.MAP_CU, capi.MAP_SLICE), painted), case["what"])
    finally:
        ctx.close()


def check_result_rejections(lib):
    ctx = capi.Context(lib, 0)
    try:
        h = ctx.upload(synthetic("72x40_ctb64")[0])
        tk = ctx.picture_maps_async(h, 2)
        out = capi.MapsInfo()
        assert lib.lib.m355_picture_maps_result(ctx.h, tk, 1, None) == INVALID, "null result"
        assert lib.lib.m355_picture_maps_result(ctx.h, tk + 1, 1, ctypes.byref(out)) == INVALID, "unknown ticket"
        assert lib.lib.m355_picture_maps_order(ctx.h, 0, None) == INVALID, "ticket 0"
        ctx.picture_maps_result(tk)
        assert lib.lib.m355_picture_maps_result(ctx.h, tk, 1, ctypes.byref(out)) == INVALID, "collected ticket"
    finally:
        ctx.close()


# 9
def check_decodes_undisturbed(lib, oracle):
    """three pictures decoded at depth 3 with a request behind each, and the same without: equal frame hashes, and the oracle's pictures"""
    o = Oracle(oracle)
    cases = [make_case(width=200, height=120, log2_ctb=4, intra_pct=30, seed=60 + k) for k in range(3)]
    want = [oracle_decode(o, pic, refs) for pic, refs in cases]
    hashes = []
    for with_maps in (True, False):
        ctx = capi.Context(lib, 0)
        try:
            ctx.set_pipeline_depth(3)
            dsts, tickets, handles = [], [], []
            for pic, refs in cases:
                rf = []
                for planes in refs:
                    rf.append(ctx.frame_create_for(pic.pp[0]))
                    ctx.frame_upload(rf[-1], planes)
                dsts.append(ctx.frame_create_for(pic.pp[0]))
                pic.dst_frame = dsts[-1]
                pic.ref_frames = [rf[i] if i < len(rf) else -1 for i in range(worklist.MAX_REF_FRAMES)]
                handles.append(ctx.upload(pic))
            for k, h in enumerate(handles):
                ctx.decode_resident(h)
                if with_maps:
                    tickets.append(ctx.picture_maps_async(h, 2))
            for k, t in enumerate(tickets):
                assert_maps(ctx.picture_maps_result(t), expected(cases[k][0], 2), "picture %d" % k)
            ctx.wait()
            hashes.append([ctx.frame_hash(d, CRC) for d in dsts])
            for k, d in enumerate(dsts):
                assert_planes_equal(ctx.frame_download(d), want[k], "picture %d %s requests" % (k, "with" if with_maps else "without"))
        finally:
            ctx.close()
    assert hashes[0] == hashes[1]


# ---- the host helper ----
def check_host_unit(lib, pic, log2_unit, maps=ALL, painted=None, step=1):
    """m355_maps_unit on every `step`-th unit of every map against the restatement"""
    want, _ = expected(pic, log2_unit, maps, painted)
    c_pic = pic.to_c()
    for m in maps:
        w = want[m]
        for uy in range(0, w.shape[0], step):
            for ux in range(0, w.shape[1], step):
                got = lib.maps_unit(pic, m, log2_unit, ux, uy, c_pic=c_pic)
                exp = w[uy, ux].tolist()
                assert got == exp, "map %s unit %d,%d at %d: %r, expected %r" % (capi.MAP_NAMES[m], ux, uy, 1 << log2_unit, got, exp)
