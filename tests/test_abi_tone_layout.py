"""m355_colour_tone (include/de265_mi355x.h) as the C compiler lays it out against capi.ColourTone: size and the offset of every field, and the
constants that go with it."""
import ctypes
import os
import subprocess

from libde265_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include <stddef.h>
#include <stdio.h>
#include "de265_mi355x.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(m355_colour_tone), offsetof(m355_colour_tone, norm), offsetof(m355_colour_tone, weights),
         offsetof(m355_colour_tone, gain), offsetof(m355_colour_tone, reserved), M355_TONE_GAIN_ONE, M355_NORM_MAXRGB, M355_NORM_LUMA, M355_TONE_BT2390,
         M355_COLOUR_OUT_KNOTS);
  return 0;
}
"""


def test_colour_tone_layout(tmp_path):
    exe = tmp_path / "tone_layout"
    subprocess.run(["gcc", "-x", "c", "-", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe)], input=SOURCE, text=True, check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = capi.ColourTone
    assert got[:5] == [ctypes.sizeof(T), T.norm.offset, T.weights.offset, T.gain.offset, T.reserved.offset] == [4896, 0, 4, 16, 4884]
    assert got[5:] == [capi.TONE_GAIN_ONE, capi.NORM_MAXRGB, capi.NORM_LUMA, capi.TONE_BT2390, capi.COLOUR_OUT_KNOTS]
    assert T.gain.size == 4 * capi.COLOUR_OUT_KNOTS and T.weights.size == 12 and T.reserved.size == 12
