"""The score -> key transform of the per-query top-k (csrc/apss_topk_key.hpp) in a stand-alone CPU program built with
AddressSanitizer and UBSan: strictly monotonic over the floats a score can be, +-0 share a key, the inverse round-trips."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "apss_topk_key.hpp"

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const float dmin = std::numeric_limits<float>::denorm_min();
  const float nmin = std::numeric_limits<float>::min();
  const float big = std::numeric_limits<float>::max();
  // strictly ascending, apart from the pair of zeros
  std::vector<float> v = {-inf, -big, -2.5f, -1.0f, std::nextafter(-1.0f, 0.0f), -0.45f, -1e-20f, -nmin, -std::nextafter(nmin, 0.0f),
                          -1e-41f, -2 * dmin, -dmin, -0.0f, 0.0f, dmin, 2 * dmin, 1e-41f, std::nextafter(nmin, 0.0f), nmin, 1e-20f,
                          0.45f, std::nextafter(1.0f, 0.0f), 1.0f, std::nextafter(1.0f, 2.0f), 2.5f, big, inf};
  int fails = 0;
  for (size_t i = 0; i + 1 < v.size(); ++i) {
    const uint32_t a = apss::topk_key(v[i]), b = apss::topk_key(v[i + 1]);
    const bool zeros = v[i] == 0.0f && v[i + 1] == 0.0f;
    if (zeros ? a != b : !(a < b)) {
      std::printf("FAIL order at %zu: %a -> %08x, %a -> %08x\n", i, v[i], a, v[i + 1], b);
      ++fails;
    }
    if (!zeros && !(v[i] < v[i + 1])) {
      std::printf("FAIL the list itself is not ascending at %zu\n", i);
      ++fails;
    }
  }
  for (float f : v) {
    const float back = apss::topk_key_inv(apss::topk_key(f));
    const uint32_t want = f == 0.0f ? 0u : bits(f);  // either zero comes back as +0.0f
    if (bits(back) != want) {
      std::printf("FAIL round trip %a -> %a\n", f, back);
      ++fails;
    }
  }
  // a sweep over every exponent and both signs: key order == float order for neighbours in bit space
  for (uint32_t e = 0; e < 255; ++e)
    for (uint32_t m : {0u, 1u, 0x400000u, 0x7fffffu}) {
      float f, g;
      const uint32_t b = (e << 23) | m, c = b + 1;
      std::memcpy(&f, &b, 4);
      std::memcpy(&g, &c, 4);
      if (std::isnan(g) ) continue;
      if (!(apss::topk_key(f) < apss::topk_key(g)) || !(apss::topk_key(-g) < apss::topk_key(-f))) {
        std::printf("FAIL sweep e=%u m=%u\n", e, m);
        ++fails;
      }
      if (bits(apss::topk_key_inv(apss::topk_key(-g))) != (c | 0x80000000u)) ++fails;
    }
  std::printf(fails ? "topk_key: %d FAILED\n" : "topk_key: PASS\n", fails);
  return fails ? 1 : 0;
}
"""


def test_key_is_monotonic_and_round_trips(tmp_path):
    src = tmp_path / "topk_key_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "topk_key_check"
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                          "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "topk_key: PASS" in run.stdout


def test_key_header_has_no_hip_include():
    txt = open(os.path.join(CSRC, "apss_topk_key.hpp")).read()
    assert "hip/" not in txt and "__HIPCC__" in txt
