"""The host side of the colour transform under AddressSanitizer and UndefinedBehaviorSanitizer: a small stand-alone program with its own main, compiled
here with g++ -fsanitize=address,undefined from csrc/colour_transform.h and csrc/colour_preset.h (the code behind m355_colour_pixel and
m355_colour_preset), builds every supported preset and runs the pixel function over the corners of its tables.  The program runs as a child process;
nothing sanitised is loaded into this interpreter, and no GPU is involved.  The sanitisers' runtimes are linked statically into the program, so it
needs nothing from the environment it is started in."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include <stdio.h>
#include <initializer_list>
#include "colour_preset.h"

static unsigned long long fold(unsigned long long h, unsigned v) { return (h ^ v) * 1099511628211ull; }

int main()
{
  static const int in_t[] = {1, 2, 6, 14, 15, 13, 8, 16, 18}, out_t[] = {1, 2, 6, 14, 15, 13, 8}, prim[] = {1, 2, 5, 6, 9};
  static const unsigned corner[] = {0, 1, 62, 63, 64, 65, 127, 128, 4095, 4096, 32767, 32768, 65471, 65472, 65534, 65535, 70000};
  const int nc = (int)(sizeof(corner) / sizeof(corner[0]));
  unsigned long long h = 1469598103934665603ull;
  int built = 0;
  m355_colour_tables* t = new m355_colour_tables;
  for (int a : in_t) for (int b : prim) for (int c : out_t) for (int d : prim) for (int tone = 0; tone < 2; tone++) for (int peak : {0, 203, 4000}) {
    m355_colour_preset_desc q = {a, b, c, d, tone, 0, peak, 0};
    if (m355_cp_build(&q, t)) { printf("preset %d %d %d %d %d %d rejected\n", a, b, c, d, tone, peak); return 1; }
    if (m355_ct_tables_check(t)) { printf("preset %d %d %d %d leaves the bounds\n", a, b, c, d); return 1; }
    built++;
    if (b != prim[built % 5] && tone) continue;                 /* (the pixel function on a part of them: the tables of the others repeat) */
    for (int samples = 0; samples < 2; samples++)
      for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j += 3) for (int k = 0; k < nc; k += 5) {
        const unsigned rgb[3] = {corner[i], corner[(i + j) % nc], corner[(j + k) % nc]};
        unsigned out[3];
        m355_ct_pixel(t, rgb, samples, out);
        for (int e = 0; e < 3; e++) { if (out[e] > (samples ? 65535u : 255u)) { printf("output %u out of range\n", out[e]); return 1; } h = fold(h, out[e]); }
      }
  }
  /* the extreme tables: every product and sum at its bound */
  for (int k = 0; k < M355_COLOUR_IN_KNOTS; k++) t->lut_in[k] = M355_COLOUR_ONE;
  for (int sign = -1; sign <= 1; sign += 2) {
    for (int k = 0; k < 9; k++) t->matrix[k] = sign * 65535;
    for (int i = 0; i < nc; i++) { const unsigned rgb[3] = {corner[i], corner[nc - 1 - i], corner[i]}; unsigned out[3]; m355_ct_pixel(t, rgb, 1, out); h = fold(h, out[0] + out[1] + out[2]); }
  }
  unsigned idx, fr;
  for (unsigned p : {0u, 1u, 63u, 64u, 65u, 127u, 128u, (unsigned)M355_COLOUR_ONE - 1u, (unsigned)M355_COLOUR_ONE}) {
    m355_ct_out_index(p, &idx, &fr);
    if (idx > (unsigned)M355_COLOUR_OUT_LAST || m355_ct_out_knot(idx) > p) { printf("index of %u\n", p); return 1; }
  }
  m355_colour_preset_desc bad = {16, 9, 16, 1, 0, 0, 0, 0};
  if (!m355_cp_build(&bad, t) || !m355_cp_build(nullptr, t) || !m355_cp_build(&bad, nullptr)) { printf("a bad descriptor was accepted\n"); return 1; }
  delete t;
  printf("ok %d presets %llx\n", built, h);
  return 0;
}
"""


def test_presets_and_pixel_function_under_asan_and_ubsan(tmp_path):
    src, exe = tmp_path / "colour_host.cc", tmp_path / "colour_host"
    src.write_text(SOURCE)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libde265_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok 9450 presets"), r.stdout + r.stderr
