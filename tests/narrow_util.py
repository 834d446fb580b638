"""Shared cases for the 16-bit coefficient entries (M355_RBF_NARROW, include/de265_mi355x.h): synthetic pictures whose levels are
forced into the range the narrow form holds, the packed pictures the device decodes, and the oracle's decode of the WIDE lists as the
expected picture (the oracle only reads the wide form).  test_emu_narrow.py (SIMT-interpreter build) and test_gpu_narrow.py run the
same cases; test_narrow_roundtrip.py checks the packers on the host."""
import functools
import hashlib

import numpy as np

from libde265_amd import capi, worklist
from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from test_emu_depths import CASES as DEPTH_CASES
from test_emu_synth import CASES as SYNTH_CASES

NARROW = worklist.RBF_NARROW


def is_narrow(pic):
    return (pic.rbs["flags"] & NARROW) != 0


def _entry_index(pic):
    """(index into pic.coeffs of every entry of every block of a WIDE picture, entry number inside its block, entries per block)"""
    assert not is_narrow(pic).any()
    n = pic.rbs["ncoeff"].astype(np.int64)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return np.repeat(pic.rbs["coeff_ofs"].astype(np.int64), n) + k, k, n


def force_levels(pic, blocks=None, seed=1):
    """A copy of the wide picture in which the levels of the chosen blocks (default: all) are values in [-128, 127], never 0; the
    positions stay."""
    out = pic.copy()
    idx, _, n = _entry_index(pic)
    chosen = np.repeat(np.ones(len(n), bool) if blocks is None else np.asarray(blocks, dtype=bool), n)
    lvl = np.random.RandomState(seed).randint(-128, 128, size=len(idx))
    lvl[lvl == 0] = 1
    co = out.coeffs
    co[idx[chosen]] = (co[idx[chosen]] & 0xFFFF) | ((lvl[chosen] & 0xFFFF).astype(np.uint32) << 16)
    return out


def keep_entries(pic, keep):
    """A copy of the wide picture with only the entries keep[...] (a boolean array over all entries, record order) left in the blocks."""
    idx, _, n = _entry_index(pic)
    out = pic.copy()
    block = np.repeat(np.arange(len(n)), n)
    n2 = np.bincount(block[keep], minlength=len(n)).astype(np.int64)
    ofs = np.cumsum(n2) - n2                                   # (record order: the packers restore any order, this one is as good)
    out.coeffs = pic.coeffs[idx[keep]].astype(np.dtype("<u4"))
    out.rbs["ncoeff"] = n2.astype(np.uint16)
    out.rbs["coeff_ofs"] = ofs.astype(np.uint32)
    return out


def poison_spare_halves(pic):
    """0xFFFF in the unused half of the last word of every narrow block with an odd count: it must never be read as an entry"""
    n = pic.rbs["ncoeff"].astype(np.int64)
    odd = is_narrow(pic) & (n % 2 == 1)
    w = pic.rbs["coeff_ofs"].astype(np.int64)[odd] + n[odd] // 2
    pic.coeffs[w] |= np.uint32(0xFFFF0000)
    return pic


# ---- how a case shapes its lists: wide picture (as generated) -> (wide picture the oracle decodes, packed picture the device decodes) ----
def _all(wide):
    wide = force_levels(wide)
    return wide, worklist.pack_narrow(wide)


def _only(select):
    def shape(wide):
        wide = force_levels(wide)
        return wide, worklist.pack_narrow(wide, blocks=select(wide.rbs))
    return shape


def _alternate(wide):
    """everything packed, then every second record widened again: narrow and wide blocks side by side in one wave"""
    wide = force_levels(wide)
    packed = worklist.pack_narrow(wide)
    return wide, worklist.unpack_narrow(packed, blocks=np.arange(len(packed.rbs)) % 2 == 1)


def _low_positions(wide):
    """32x32 blocks whose positions are all below 256"""
    idx, _, n = _entry_index(wide)
    big = np.repeat(wide.rbs["log2_size"] == 5, n)
    wide = force_levels(keep_entries(wide, ~big | ((wide.coeffs[idx] & 0xFFFF) < 256)))
    return wide, worklist.pack_narrow(wide)


def _bin(s):
    """one size bin alone (the 32x32 blocks keep their low positions only, or none of them could take the form)"""
    def shape(wide):
        wide, _ = _low_positions(wide)
        return wide, worklist.pack_narrow(wide, blocks=wide.rbs["log2_size"] == s + 2)
    return shape


def _one_high_position(wide):
    """the twin: one entry of the first such block sits at position 256 or above — the block must stay wide"""
    wide, _ = _low_positions(wide)
    i = int(np.flatnonzero((wide.rbs["log2_size"] == 5) & (wide.rbs["ncoeff"] > 0))[0])
    o = int(wide.rbs["coeff_ofs"][i])
    wide.coeffs[o] = (wide.coeffs[o] & np.uint32(0xFFFF0000)) | np.uint32(1023)      # (1023 is not among positions < 256: no duplicate)
    wide.meta["high_block"] = i
    return wide, worklist.pack_narrow(wide)


def _counts(wide):
    """blocks of 1, 2, 3, ... 6 entries: ncoeff = 1, odd and even"""
    _, k, n = _entry_index(wide)
    limit = np.repeat(1 + np.arange(len(n)) % 6, n)
    wide = force_levels(keep_entries(wide, k < limit))
    return wide, worklist.pack_narrow(wide)


def _last_record_ends_list(wide):
    """the LAST record's entries moved to the end of the list and cut to an odd count: narrow, it ends in the list's last word, and
    coeff_ofs + ncoeff lies beyond n_coeffs"""
    wide = force_levels(wide)
    last = len(wide.rbs) - 1
    n = int(wide.rbs["ncoeff"][last])
    assert n >= 3
    n -= 1 - n % 2
    o = int(wide.rbs["coeff_ofs"][last])
    wide.coeffs = np.concatenate([wide.coeffs, wide.coeffs[o:o + n]]).astype(np.dtype("<u4"))
    wide.rbs["coeff_ofs"][last] = len(wide.coeffs) - n
    wide.rbs["ncoeff"][last] = n
    wide = worklist.unpack_narrow(wide)                        # (compacted: the hole the move left is gone)
    return wide, worklist.pack_narrow(wide)


CCP = dict(width=64, height=64, bit_depth=8, seed=34, chroma_format=3, intra_pct=30, features=32, fixed_cu_log2=4, cbf_pct=100)
ALL_SIZES = dict(width=192, height=128, bit_depth=8, seed=11)

# name -> (generator configuration, shaping)
CASES = {
    "8x8": (dict(width=8, height=8, bit_depth=8, seed=26, log2_ctb=4, cbf_pct=100), _all),
    "72x24_9bit_deferred": (dict(width=72, height=24, bit_depth=9, seed=27, log2_ctb=4, intra_pct=50), _all),
    "ccp_luma_narrow": (CCP, _only(lambda rbs: rbs["cidx"] == 0)),
    "ccp_chroma_narrow": (CCP, _only(lambda rbs: rbs["cidx"] != 0)),
    "ccp_both_narrow": (CCP, _all),
    "416x240_8bit_alternate": (dict(width=416, height=240, bit_depth=8, seed=21), _alternate),
    "416x240_10bit_alternate": (dict(width=416, height=240, bit_depth=10, seed=22), _alternate),
    "32x32_low_positions": (dict(width=64, height=64, bit_depth=8, seed=30, fixed_cu_log2=6, cbf_pct=100), _low_positions),
    "32x32_one_high_position": (dict(width=64, height=64, bit_depth=8, seed=30, fixed_cu_log2=6, cbf_pct=100), _one_high_position),
    "counts_1_odd_even": (dict(width=64, height=64, bit_depth=8, seed=36, cbf_pct=100), _counts),
    "last_record_ends_list": (dict(width=64, height=64, bit_depth=8, seed=37, cbf_pct=100, intra_pct=30), _last_record_ends_list),
    "16bit_deferred": (DEPTH_CASES[1], _all),
}
for _c in SYNTH_CASES:
    if _c["seed"] in (41, 42, 43, 44):                         # transform skip, bypass, RDPCM, rotation, pre-scaled levels
        CASES["features_seed%d" % _c["seed"]] = (_c, _all)
for _s in range(4):                                            # each size bin on its own (one picture, one expected decode)
    CASES["bin%d_only" % _s] = (ALL_SIZES, _bin(_s))
SHARDED = (dict(width=256, height=128, bit_depth=8, seed=41, tile_cols=2, tile_rows=1), _alternate)     # two ranks (CPU tier)


@functools.lru_cache(maxsize=None)
def _built(name):
    cfg, shape = SHARDED if name == "sharded" else CASES[name]
    pic, refs = make_case(**cfg)
    wide, packed = shape(pic)
    assert is_narrow(packed).any(), "nothing was packed: the case would pass without the feature"
    assert not is_narrow(wide).any()
    return wide, poison_spare_halves(packed), refs


_expected = {}


def case(name, oracle):
    """-> (wide picture, packed picture, reference planes, expected planes = the oracle's decode of the wide lists); built once, and
    cases that pack the same wide lists differently share one oracle decode"""
    wide, packed, refs = _built(name)
    key = hashlib.sha1(repr(sorted(wide.meta["cfg"].items())).encode() + wide.rbs.tobytes() + wide.coeffs.tobytes()).hexdigest()
    if key not in _expected:
        _expected[key] = oracle_decode(Oracle(oracle), wide, refs)
    return wide, packed, refs, _expected[key]


def decode(ctx, pic, refs, in_place, fill=None):
    """One decode through m355_submit_picture: lists copied by the library, or (in_place) recorded into the arena of m355_arena_begin —
    the path whose records the DEVICE validates.  fill: (luma, chroma) values the destination holds beforehand.
    -> (planes of the destination afterwards, the M355Error the submit or the wait raised or None)"""
    pp = pic.pp[0]
    handles = []
    for planes in refs:
        f = ctx.frame_create_for(pp)
        ctx.frame_upload(f, planes)
        handles.append(f)
    dst = ctx.frame_create_for(pp)
    if fill:
        ctx.frame_fill(dst, *fill)
    pic.dst_frame = dst
    pic.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
    err = None
    try:
        if in_place:
            ctx.submit_in_place(pic, fill_threads=1)
        else:
            ctx.submit(pic)
        ctx.wait()
    except capi.M355Error as e:
        err = e
    out = ctx.frame_download(dst)
    for f in handles + [dst]:
        ctx.frame_destroy(f)
    return out, err


def check_case(ctx, oracle, name, in_place):
    """the device's decode of the packed picture == the oracle's decode of the wide lists, and the case holds what it is there for"""
    wide, packed, refs, want = case(name, oracle)
    rbs, nar, n = packed.rbs, is_narrow(packed), packed.rbs["ncoeff"].astype(np.int64)
    assert nar.any()
    if name.startswith("ccp_"):
        ccp = np.flatnonzero((rbs["cidx"] > 0) & (((rbs["matrix_id"] >> 4) & 7) != 0))
        luma = ccp - np.where(rbs["matrix_id"][ccp] & 8, 2, 1)
        assert len(ccp) and (rbs["cidx"][luma] == 0).all()
        assert nar[luma].all() == (name != "ccp_chroma_narrow") and nar[ccp].any() == (name != "ccp_luma_narrow")
    if name.endswith("_alternate"):
        assert (nar[:-1] != nar[1:]).sum() > len(nar) // 4         # narrow and wide records side by side
    if name == "32x32_low_positions":
        assert nar[rbs["log2_size"] == 5].any()
    if name == "32x32_one_high_position":
        assert not nar[wide.meta["high_block"]] and nar[rbs["log2_size"] == 5].any()
    if name == "counts_1_odd_even":
        assert (nar & (n == 1)).any() and (nar & (n % 2 == 1) & (n > 1)).any() and (nar & (n % 2 == 0)).any()
    if name == "last_record_ends_list":
        last = rbs[-1]
        assert nar[-1] and int(last["coeff_ofs"]) + (int(last["ncoeff"]) + 1) // 2 == len(packed.coeffs) < int(last["coeff_ofs"]) + int(last["ncoeff"])
    if name.startswith("bin"):
        assert (rbs["log2_size"][nar] == int(name[3]) + 2).all()
    got, err = decode(ctx, packed, refs, in_place)
    assert err is None, err
    assert_planes_equal(got, want, "%s (%s lists)" % (name, "recorded in place" if in_place else "copied"))


def check_rejection(ctx, oracle, in_place):
    """A narrow block whose last word lies one beyond the list is refused (M355_ERR_INVALID, destination untouched) — by the host's
    check of copied lists, by the device's of lists recorded in place; the same block one word lower (it ends in the last word) decodes."""
    wide, packed, refs, want = case("last_record_ends_list", oracle)
    bad = packed.copy()
    bad.coeffs = bad.coeffs[:-1]                                   # coeff_ofs + (ncoeff + 1) / 2 == n_coeffs + 1
    last = bad.rbs[-1]
    assert int(last["coeff_ofs"]) + (int(last["ncoeff"]) + 1) // 2 == len(bad.coeffs) + 1 and is_narrow(bad)[-1]
    got, err = decode(ctx, bad, refs, in_place, fill=(77, 99))
    assert err is not None and err.code == 3, "a narrow block beyond the list was not refused"      # M355_ERR_INVALID
    assert ("rb" in str(err)) and all((pl == (77 if c == 0 else 99)).all() for c, pl in enumerate(got)), "the refused picture's destination was written"
    got, err = decode(ctx, packed, refs, in_place, fill=(77, 99))
    assert err is None, err
    assert_planes_equal(got, want, "block ending in the list's last word")
