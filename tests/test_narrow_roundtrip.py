"""The packers of the 16-bit coefficient entries (M355_RBF_NARROW) on the host, no device: worklist.unpack_narrow undoes
worklist.pack_narrow exactly — on every case of narrow_util.py and on the recorded girlshy lists — and m355_pack_narrow (the library's,
host only) agrees with the numpy packer word for word."""
import numpy as np
import pytest

import narrow_util
from golden_io import load_gold
from libde265_amd import capi, worklist

NAMES = list(narrow_util.CASES) + ["sharded"]
GOLD = ["girlshy_full", "girlshy_nolf", "girlshy_nosao", "girlshy_nodeblk"]


def same_lists(a, b):
    return np.array_equal(a.rbs, b.rbs) and np.array_equal(a.coeffs, b.coeffs) and list(a.rb_count) == list(b.rb_count) and \
        a.coeffs.dtype == b.coeffs.dtype == np.dtype("<u4")


@pytest.mark.parametrize("name", NAMES)
def test_unpack_inverts_pack(name):
    wide, packed, refs = narrow_util._built(name)
    assert narrow_util.is_narrow(packed).any() and len(packed.coeffs) < len(wide.coeffs)
    assert same_lists(worklist.unpack_narrow(packed), wide)
    assert same_lists(worklist.unpack_narrow(worklist.pack_narrow(wide)), wide)
    # the words every block occupies tile the packed list: nothing overlaps, nothing is left over
    words, ofs = worklist.rb_words(packed.rbs), packed.rbs["coeff_ofs"].astype(np.int64)
    order = np.argsort(ofs, kind="stable")
    assert np.array_equal(ofs[order], np.cumsum(words[order]) - words[order]) and int(words.sum()) == len(packed.coeffs)


@pytest.mark.parametrize("gold", GOLD)
def test_unpack_inverts_pack_on_recorded_lists(gold):
    hdr, pics = load_gold(gold + ".m355gold.gz")
    before = after = 0
    for pic in pics:
        packed = worklist.pack_narrow(pic)
        assert same_lists(worklist.unpack_narrow(packed), pic)
        before += len(pic.coeffs); after += len(packed.coeffs)
    print("%s: %d coefficient words, %d packed (%.1f %%)" % (gold, before, after, 100.0 * after / before))
    assert after < before          # a real stream: most of its blocks take the form


@pytest.mark.parametrize("name", NAMES)
def test_library_packer_agrees_with_numpy(name):
    lib = capi.Library()           # (loads without a device; m355_pack_narrow makes no GPU call)
    wide, packed, refs = narrow_util._built(name)
    assert same_lists(lib.pack_narrow(wide), worklist.pack_narrow(wide))


def test_library_packer_agrees_with_numpy_on_recorded_lists():
    lib = capi.Library()
    hdr, pics = load_gold("girlshy_full.m355gold.gz")
    for pic in pics:
        assert same_lists(lib.pack_narrow(pic), worklist.pack_narrow(pic))


def test_library_packer_refuses_a_range_outside_the_list():
    lib = capi.Library()
    wide, packed, refs = narrow_util._built("8x8")
    bad = wide.copy()
    bad.rbs["coeff_ofs"][0] = len(bad.coeffs)
    with pytest.raises(capi.M355Error) as e:
        lib.pack_narrow(bad)
    assert e.value.code == 3       # M355_ERR_INVALID
