"""The host side of the tone objects under AddressSanitizer and UndefinedBehaviorSanitizer: a small stand-alone program with its own main, compiled
here with g++ -fsanitize=address,undefined from csrc/colour_transform.h and csrc/colour_preset.h (the code behind m355_colour_pixel_tone and
m355_colour_preset_tone), builds every supported tone preset and runs the pixel function over the corners of its tables, as
test_colour_host_sanitized.py does for the plain objects.  The program runs as a child process; nothing sanitised is loaded into this interpreter, and
no GPU is involved.  The sanitisers' runtimes are linked statically into the program, so it needs nothing from the environment it is started in."""
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
  static const int in_t[] = {1, 13, 8, 16, 18}, out_t[] = {1, 13, 8}, prim[] = {1, 2, 5, 6, 9};
  static const unsigned corner[] = {0, 1, 62, 63, 64, 65, 127, 128, 4095, 4096, 32767, 32768, 65471, 65472, 65534, 65535, 70000};
  const int nc = (int)(sizeof(corner) / sizeof(corner[0]));
  unsigned long long h = 1469598103934665603ull;
  int built = 0;
  m355_colour_tables* t = new m355_colour_tables;
  m355_colour_tone* q = new m355_colour_tone;
  for (int a : in_t) for (int b : prim) for (int c : out_t) for (int d : prim) for (int tone = 0; tone < 3; tone++) for (int norm = 0; norm < 2; norm++)
    for (int peak : {0, 203, 4000}) {
      m355_colour_preset_desc desc = {a, b, c, d, tone, 0, peak, 0};
      if (m355_cp_build_tone(&desc, norm, t, q)) { printf("preset %d %d %d %d %d %d %d rejected\n", a, b, c, d, tone, norm, peak); return 1; }
      if (m355_ct_tables_check(t) || m355_ct_tone_check(q)) { printf("preset %d %d %d %d %d %d %d leaves the bounds\n", a, b, c, d, tone, norm, peak); return 1; }
      built++;
      if (b != prim[built % 5] || d != 1) continue;              /* (the pixel function on a part of them: the tables of the others repeat) */
      for (int samples = 0; samples < 2; samples++)
        for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j += 3) for (int k = 0; k < nc; k += 5) {
          const unsigned rgb[3] = {corner[i], corner[(i + j) % nc], corner[(j + k) % nc]};
          unsigned out[3];
          m355_ct_pixel_tone(t, q, rgb, samples, out);
          for (int e = 0; e < 3; e++) { if (out[e] > (samples ? 65535u : 255u)) { printf("output %u out of range\n", out[e]); return 1; } h = fold(h, out[e]); }
        }
    }
  for (int a : {2, 6, 14, 15}) {                                 /* the other code points of transfer 1: one path, built once each */
    m355_colour_preset_desc desc = {a, 9, a, 2, 2, 0, 1000, 0};
    if (m355_cp_build_tone(&desc, 1, t, q) || m355_ct_tone_check(q)) { printf("transfer %d rejected\n", a); return 1; }
  }
  /* the extreme tables: every product and sum at its bound — P = ONE in every channel, the weights at +-65535, every gain GAIN_ONE, then 0 */
  for (int k = 0; k < M355_COLOUR_IN_KNOTS; k++) t->lut_in[k] = M355_COLOUR_ONE;
  q->norm = M355_NORM_LUMA;
  for (int sign = -1; sign <= 1; sign += 2) for (unsigned gain : {(unsigned)M355_TONE_GAIN_ONE, 0u}) {
    for (int k = 0; k < 9; k++) t->matrix[k] = sign * 65535;
    for (int k = 0; k < 3; k++) q->weights[k] = -sign * 65535;
    for (int k = 0; k < M355_COLOUR_OUT_KNOTS; k++) q->gain[k] = gain;
    if (m355_ct_tone_check(q)) { printf("the extreme tone leaves the bounds\n"); return 1; }
    for (int i = 0; i < nc; i++) { const unsigned rgb[3] = {corner[i], corner[nc - 1 - i], corner[i]}; unsigned out[3]; m355_ct_pixel_tone(t, q, rgb, 1, out); h = fold(h, out[0] + out[1] + out[2]); }
  }
  if (m355_ct_gain(M355_TONE_GAIN_ONE, M355_TONE_GAIN_ONE, 255) != (unsigned)M355_TONE_GAIN_ONE || m355_ct_apply(M355_COLOUR_ONE, M355_TONE_GAIN_ONE) != (unsigned)M355_COLOUR_ONE) {
    printf("the largest operands\n"); return 1;
  }
  q->gain[5] = M355_TONE_GAIN_ONE + 1;
  if (m355_ct_tone_check(q) != 3) { printf("a gain above one was accepted\n"); return 1; }
  m355_colour_preset_desc bad = {16, 9, 16, 1, 2, 0, 0, 0}, ks = {16, 9, 1, 1, 2, 5, 10000, 0}, ok = {16, 9, 1, 1, 2, 203, 1000, 0};
  if (!m355_cp_build_tone(&bad, 0, t, q) || !m355_cp_build_tone(&ks, 0, t, q) || !m355_cp_build_tone(&ok, 2, t, q) || !m355_cp_build_tone(nullptr, 0, t, q) ||
      !m355_cp_build_tone(&ok, 0, nullptr, q) || !m355_cp_build_tone(&ok, 0, t, nullptr) || !m355_cp_build(&ok, t) || m355_cp_build_tone(&ok, 0, t, q)) {
    printf("a bad descriptor was accepted, or a good one rejected\n"); return 1;
  }
  delete t;
  delete q;
  printf("ok %d presets %llx\n", built, h);
  return 0;
}
"""


def test_tone_presets_and_pixel_function_under_asan_and_ubsan(tmp_path):
    src, exe = tmp_path / "tone_host.cc", tmp_path / "tone_host"
    src.write_text(SOURCE)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "libde265_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok 6750 presets"), r.stdout + r.stderr
