"""Content that makes the deblocking filter WORK, and a census of what it did (tests/test_deblock_smooth.py).

The generator's reference planes (csrc/synth.c m355_synth_ref_plane: box-blurred noise + a ramp) have second differences above beta
nearly everywhere, so `d < beta` (deblock.cc:517) is false on almost every luma edge segment of the synthetic suites and neither the
normal nor the strong filter runs.  smooth_refs() replaces the left two thirds of every reference plane with a low-slope ramp: the
prediction there is smooth, block borders are small steps, and edges with no filter, the normal filter and the strong filter meet in
one picture — at tile and slice borders too; the right third stays as generated.

deblock_census() classifies what the filter changed from the planes before and after it alone (no counter in any kernel): on the
8-sample grid a sample at distance i from an edge is p_i / q_i of that edge, the two passes change p0..p2 / q0..q2 only, so a
changed sample whose distance m from the nearest grid line (in x or y) is 1 is p1 / q1 of the normal (dEp / dEq) or the strong
filter, and one at m >= 2 can only be p2 / q2 of the strong filter (fallback-deblk.h:61-76)."""
import numpy as np

from synth_util import make_case


def ramp_plane(h, w, bd, dtype):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.int64)
    v = (1 << bd) // 4 + (((xx + 2 * yy) << (bd - 8)) >> 2)
    return np.clip(v, 0, (1 << bd) - 1).astype(dtype)


def smooth_refs(refs, bd_luma, bd_chroma):
    """the reference planes with the left two thirds of their columns replaced by a ramp of 1/4 (x) and 1/2 (y) of an 8-bit step per sample"""
    out = []
    for planes in refs:
        new = []
        for c, p in enumerate(planes):
            h, w = p.shape
            q = p.copy()
            n = (2 * w) // 3
            q[:, :n] = ramp_plane(h, w, bd_chroma if c else bd_luma, p.dtype)[:, :n]
            new.append(q)
        out.append(new)
    return out


def make_smooth_case(**cfg):
    """synth_util.make_case with the references smoothed"""
    pic, refs = make_case(**cfg)
    pp = pic.pp[0]
    return pic, smooth_refs(refs, int(pp["bit_depth_luma"]), int(pp["bit_depth_chroma"]))


def _grid_distance(n):
    r = np.arange(n) & 7
    return np.minimum(r, 7 - r)          # q0 / p0: 0, q1 / p1: 1, q2 / p2: 2, q3 / p3 (never written): 3


def _one_sided(ch):
    """4-sample segments of the vertical 8-grid edges of `ch` (bool, changed) with changes on exactly one side.  A segment is judged on
    the one line of its four that the OTHER pass cannot have written (distance 3 from the horizontal grid lines: lines 3 and 4 of every 8),
    so a change there belongs to this edge; and it counts only where the changed side's sample AT the edge changed: a two-sided normal
    filter moves p0 and q0 by the same delta, but with delta == 0 and dEp != dEq it moves p1 or q1 alone, which is not what is counted."""
    h, w = ch.shape
    n = 0
    for y in range(0, h, 4):
        line = y + 3 if (y & 7) == 0 else y
        if line >= h:
            continue
        for x in range(8, w, 8):
            cp, cq = ch[line, x - 3:x].any(), ch[line, x:x + 3].any()
            n += int((ch[line, x - 1] and not cq) or (ch[line, x] and not cp))
    return n


def deblock_census(pre, post):
    """pre / post: the planes before and after deblocking -> per plane dict(samples, changed, m1, m2, one_sided)"""
    out = []
    for a, b in zip(pre, post):
        ch = a != b
        h, w = ch.shape
        m = np.minimum(_grid_distance(h)[:, None], _grid_distance(w)[None, :])
        out.append(dict(samples=h * w, changed=int(ch.sum()), m1=int((ch & (m == 1)).sum()), m2=int((ch & (m >= 2)).sum()),
                        one_sided=_one_sided(ch) + _one_sided(ch.T)))
    return out
