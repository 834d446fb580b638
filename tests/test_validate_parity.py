"""The record checks of the work lists run in two places: on the host for lists the library copies (validate(), runtime_upload.hip)
and on the device for lists recorded in place (k_validate, k_meta.hip).  Both call the predicates of csrc/record_checks.h; this
file pins what that buys: a record one path rejects is rejected by the other, under the same list name and — where the two paths
number records alike — the same index.  One corruption per clause of the six predicates, each the nearest value that must fail.

Numbering differs in two lists (include/de265_mi355x.h, m355_decode_status): the host numbers an rb across the four size bins, the
device inside its bin; the device checks the sorted copy of ibs.  For those the name alone is compared.  A corrupt intra block whose
size or component is out of range is caught earlier still, by the host's walk over the CTB table, on BOTH paths ("ctb").

CPU tier: SIMT-interpreter build.  GPU tier: the product library."""
import re

import numpy as np
import pytest

from oracle_py import Oracle
from synth_util import assert_planes_equal, make_case, oracle_decode
from test_emu_picture import emu_lib  # noqa: F401  (fixture)
from libde265_amd import capi, synth, worklist

# 120x56 with 64x64 CTBs: the picture ends inside its last CTB column and row, so a block pushed past the picture's edge still lies
# inside its CTB — the record check is what must catch it.  Every list is populated: both reference lists, explicit weights, all four
# residual size bins (deferred ones among them), intra blocks with residual, PCM, scaling lists.
CASE = dict(width=120, height=56, bit_depth=8, seed=6, intra_pct=40, weighted_pct=40, features=synth.SYN_SCALING_LIST | synth.SYN_PCM)
FILL = (77, 99)
NARROW = 1 << 5                       # M355_RBF_NARROW


def first(mask, what):
    idx = np.flatnonzero(mask)
    assert len(idx), "the case holds no %s" % what
    return int(idx[0])


def comp_dim(pic, cidx, axis):
    """width (axis 0) / height (axis 1) of the component's plane"""
    pp = pic.pp[0]
    return worklist.plane_dims(int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]))[cidx][axis]


def rb_bins(pic):
    return np.repeat(np.arange(4), pic.rb_count)


def any_rec(pic, a):
    return len(a) // 2


def weighted_on(l):
    return lambda pic, a: first(((a["flags"] & worklist.PBF_WEIGHTED) != 0) & ((a["flags"] & (worklist.PBF_MC_L0 << l)) != 0), "weighted PB on list %d" % l)


def on_list0(pic, a):
    return first((a["flags"] & worklist.PBF_MC_L0) != 0, "PB predicted from list 0")


def set_field(field, value, sub=None):
    def f(pic, a, i):
        v = value(pic, a, i) if callable(value) else value
        if sub is None:
            a[field][i] = v
        else:
            a[field][i][sub] = v
    return f


def rb_words(a, i, narrow):
    return (int(a["ncoeff"][i]) + 1) // 2 if narrow else int(a["ncoeff"][i])


def rb_narrow_past_end(pic, a, i):
    a["flags"][i] |= NARROW
    a["coeff_ofs"][i] = len(pic.coeffs) + 1 - rb_words(a, i, True)


def ib_sq(a, i):
    return 1 << (2 * int(a["log2_size"][i]))


# (id, list, message name, record to corrupt, corruption).  One row per clause of record_checks.h.
ROWS = [
    ("cu-size-below-min-cb", "cus", "cu", any_rec, set_field("log2_size", lambda pic, a, i: int(pic.pp[0]["log2_min_cb_size"]) - 1)),
    ("cu-size-above-ctb", "cus", "cu", any_rec, set_field("log2_size", lambda pic, a, i: int(pic.pp[0]["log2_ctb_size"]) + 1)),
    ("cu-x-width", "cus", "cu", any_rec, set_field("x", lambda pic, a, i: int(pic.pp[0]["width"]))),
    ("cu-y-height", "cus", "cu", any_rec, set_field("y", lambda pic, a, i: int(pic.pp[0]["height"]))),
    ("cu-pred-mode-3", "cus", "cu", any_rec, set_field("pred_mode", 3)),
    ("cu-part-mode-8", "cus", "cu", any_rec, set_field("part_mode", 8)),
    ("tu-log2-1", "tus", "tu", any_rec, set_field("log2_size", 1)),
    ("tu-log2-7", "tus", "tu", any_rec, set_field("log2_size", 7)),
    ("tu-x-width", "tus", "tu", any_rec, set_field("x", lambda pic, a, i: int(pic.pp[0]["width"]))),
    ("tu-y-height", "tus", "tu", any_rec, set_field("y", lambda pic, a, i: int(pic.pp[0]["height"]))),
    ("pb-w-0", "pbs", "pb", any_rec, set_field("w", 0)),
    ("pb-w-68", "pbs", "pb", any_rec, set_field("w", 68)),
    ("pb-w-6", "pbs", "pb", any_rec, set_field("w", 6)),
    ("pb-right-edge-plus-4", "pbs", "pb", lambda pic, a: first(a["x"].astype(int) + a["w"] == int(pic.pp[0]["width"]), "PB at the right edge"),
     set_field("x", lambda pic, a, i: int(a["x"][i]) + 4)),
    ("pb-no-list", "pbs", "pb", any_rec, set_field("flags", lambda pic, a, i: int(a["flags"][i]) & ~(worklist.PBF_MC_L0 | worklist.PBF_MC_L1))),
    ("pb-ref-slot-minus-1", "pbs", "pb", on_list0, set_field("ref_slot", -1, 0)),
    ("pb-ref-slot-max", "pbs", "pb", on_list0, set_field("ref_slot", worklist.MAX_REF_FRAMES, 0)),
    ("pb-ref-slot-empty", "pbs", "pb", on_list0, set_field("ref_slot", lambda pic, a, i: pic.meta["cfg"]["n_refs"], 0)),      # ref_frames[n_refs] = -1
    ("pb-weight-index", "pbs", "pb", weighted_on(1), set_field("wt_idx", lambda pic, a, i: len(pic.wts), 1)),
    ("wt-luma-log2wd-0", "wts", "weight", any_rec, set_field("log2wd_luma", 0)),
    ("wt-luma-log2wd-32", "wts", "weight", any_rec, set_field("log2wd_luma", 32)),
    ("wt-chroma-log2wd-0", "wts", "weight", any_rec, set_field("log2wd_chroma", 0)),
    ("rb-log2-of-another-bin", "rbs", "rb", lambda pic, a: first(rb_bins(pic) == 1, "8x8 residual block"), set_field("log2_size", 2)),
    ("rb-cidx-3", "rbs", "rb", any_rec, set_field("cidx", 3)),
    ("rb-kind-4", "rbs", "rb", any_rec, set_field("kind", 4)),
    ("rb-chroma-x-past-width", "rbs", "rb", lambda pic, a: first(a["cidx"] > 0, "chroma residual block"),
     set_field("x", lambda pic, a, i: comp_dim(pic, int(a["cidx"][i]), 0) - (1 << int(a["log2_size"][i])) + 1)),
    ("rb-coeff-range", "rbs", "rb", lambda pic, a: first(a["ncoeff"] > 0, "coded residual block"),
     set_field("coeff_ofs", lambda pic, a, i: len(pic.coeffs) + 1 - rb_words(a, i, False))),
    ("rb-coeff-range-narrow-odd", "rbs", "rb", lambda pic, a: first((a["ncoeff"] % 2 == 1) & (a["ncoeff"] > 1), "block with an odd entry count"), rb_narrow_past_end),
    ("rb-deferred-residual-range", "rbs", "rb", lambda pic, a: first((a["flags"] & worklist.RBF_DEFERRED) != 0, "deferred residual block"),
     set_field("res_ofs", lambda pic, a, i: pic.res_len + 1 - ib_sq(a, i))),
    ("rb-matrix-id-6", "rbs", "rb", any_rec, set_field("matrix_id", 6)),
    ("rb-dst-8x8", "rbs", "rb", lambda pic, a: first(rb_bins(pic) == 1, "8x8 residual block"), set_field("kind", worklist.RK_DST)),
    ("ib-log2-1", "ibs", "ctb", any_rec, set_field("log2_size", 1)),
    ("ib-log2-6", "ibs", "ctb", any_rec, set_field("log2_size", 6)),
    ("ib-log2-255", "ibs", "ctb", any_rec, set_field("log2_size", 255)),
    ("ib-cidx-3", "ibs", "ctb", any_rec, set_field("cidx", 3)),
    ("ib-mode-35", "ibs", "ib", any_rec, set_field("mode", 35)),
    # (the block that ends at its plane's right edge: one sample further it covers the same 4x4 units of its CTB, no other block's)
    ("ib-x-past-width", "ibs", "ib", lambda pic, a: first(a["x"].astype(int) + (1 << a["log2_size"].astype(int)) ==
                                                          np.array([comp_dim(pic, int(c), 0) for c in a["cidx"]]), "intra block at the right edge"),
     set_field("x", lambda pic, a, i: int(a["x"][i]) + 1)),
    ("ib-residual-range", "ibs", "ib", lambda pic, a: first((a["flags"] & worklist.IBF_HAS_RESIDUAL) != 0, "intra block with residual"),
     set_field("res_ofs", lambda pic, a, i: pic.res_len + 1 - ib_sq(a, i))),
    ("ib-pcm-range", "ibs", "ib", lambda pic, a: first((a["flags"] & worklist.IBF_PCM) != 0, "PCM block"),
     set_field("res_ofs", lambda pic, a, i: len(pic.pcm) + 1 - ib_sq(a, i))),
]
SAME_INDEX = ("cu", "tu", "pb", "weight")            # the lists both paths number alike
RECORD = re.compile(r"\b(ctb|cu|tu|pb|weight|rb|ib) (\d+)\b")


class Rig:
    """one context at pipeline depth 1 with the case's references uploaded, shared by the rows of a tier"""

    def __init__(self, lib, oracle):
        self.lib = lib
        pic, refs = make_case(**CASE)
        self.pp = pic.pp[0]
        self.want = oracle_decode(Oracle(oracle), pic, refs)
        self.ctx = capi.Context(lib, 0)
        self.ctx.set_pipeline_depth(1)
        handles = []
        for planes in refs:
            f = self.ctx.frame_create_for(self.pp)
            self.ctx.frame_upload(f, planes)
            handles.append(f)
        self.ref_frames = [handles[i] if i < len(handles) else -1 for i in range(worklist.MAX_REF_FRAMES)]
        self.dst = self.ctx.frame_create_for(self.pp)

    def picture(self):
        pic = make_case(**CASE)[0]
        pic.ref_frames = self.ref_frames
        pic.dst_frame = self.dst
        return pic

    def host_path(self, pic):
        """the copying submit -> (status, message)"""
        try:
            self.ctx.submit(pic)
            self.ctx.wait()
        except capi.M355Error as e:
            return e.code, self.lib.error()
        return 0, ""

    def device_path(self, pic):
        """lists recorded in place -> (status, message); what only the host can check (the CTB walk) fails the submit itself"""
        try:
            self.ctx.submit_in_place(pic, fill_threads=1)
        except capi.M355Error as e:
            return e.code, self.lib.error()
        sn = self.ctx.last_serial()
        st = self.ctx.decode_status(sn)
        while st == 6:                                      # M355_ERR_BUSY
            st = self.ctx.decode_status(sn)
        return st, self.lib.error() if st else ""

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def rigs():
    made = {}
    yield made
    for r in made.values():
        r.close()


def check_case_covers_every_list(pic):
    bins = rb_bins(pic)
    assert all(len(getattr(pic, n)) for n in ("cus", "tus", "pbs", "wts", "ibs", "pcm")) and all(c > 0 for c in pic.rb_count)
    assert ((pic.rbs["flags"] & worklist.RBF_DEFERRED) != 0).any() and len(bins) == len(pic.rbs)
    assert all(((pic.pbs["flags"] & (worklist.PBF_MC_L0 << l)) != 0).any() for l in range(2)) and ((pic.pbs["flags"] & worklist.PBF_WEIGHTED) != 0).any()
    assert ((pic.ibs["flags"] & worklist.IBF_HAS_RESIDUAL) != 0).any() and ((pic.ibs["flags"] & worklist.IBF_PCM) != 0).any()
    assert (int(pic.pp[0]["flags"]) & worklist.PF_SCALING_LIST) and pic.scaling_factors is not None
    assert int(pic.pp[0]["width"]) <= 128 and int(pic.pp[0]["height"]) <= 64


def run_clean(rig):
    pic = rig.picture()
    check_case_covers_every_list(pic)
    for name, path in (("copying submit", rig.host_path), ("in-place submit", rig.device_path)):
        rig.ctx.frame_fill(rig.dst, *FILL)
        st, msg = path(pic)
        assert st == 0, "%s rejected the clean picture: %s" % (name, msg)
        rig.ctx.wait()
        assert_planes_equal(rig.ctx.frame_download(rig.dst), rig.want, name)


def run_row(rig, row):
    _, lst, name, pick, mutate = row
    pic = rig.picture()
    arr = getattr(pic, lst).copy()
    i = pick(pic, arr)
    mutate(pic, arr, i)
    setattr(pic, lst, arr)
    host_st, host_msg = rig.host_path(pic)
    rig.ctx.frame_fill(rig.dst, *FILL)
    dev_st, dev_msg = rig.device_path(pic)
    print("host: %d %r\ndevice: %d %r" % (host_st, host_msg, dev_st, dev_msg))
    assert host_st == 3, "the copying submit did not reject: %d %s" % (host_st, host_msg)     # M355_ERR_INVALID
    assert dev_st == 3, "the in-place submit did not reject: %d %s" % (dev_st, dev_msg)
    h, d = RECORD.search(host_msg), RECORD.search(dev_msg)
    assert h and d, (host_msg, dev_msg)
    assert h.group(1) == d.group(1) == name, (host_msg, dev_msg)
    if name in SAME_INDEX:
        assert int(h.group(2)) == int(d.group(2)) == i, (host_msg, dev_msg)
    rig.ctx.wait()                                          # (everything was reported through the status already)
    planes = rig.ctx.frame_download(rig.dst)
    assert all((pl == FILL[0 if c == 0 else 1]).all() for c, pl in enumerate(planes)), "a rejected picture's kernels wrote its destination frame"


IDS = [r[0] for r in ROWS]


def rig_for(rigs, tier, lib, oracle):
    if tier not in rigs:
        rigs[tier] = Rig(lib(), oracle)
    return rigs[tier]


def test_clean_picture_emulated(emu_lib, oracle, rigs):  # noqa: F811
    run_clean(rig_for(rigs, "emu", lambda: emu_lib, oracle))


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_rejection_parity_emulated(emu_lib, oracle, rigs, row):  # noqa: F811
    run_row(rig_for(rigs, "emu", lambda: emu_lib, oracle), row)


@pytest.mark.gpu
def test_clean_picture_gpu(oracle, rigs):
    run_clean(rig_for(rigs, "gpu", capi.Library, oracle))


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_rejection_parity_gpu(oracle, rigs, row):
    run_row(rig_for(rigs, "gpu", capi.Library, oracle), row)
