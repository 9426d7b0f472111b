"""The per-id decision of ``quant_tbe_remap_indices`` (``quant_remap_id`` in
ops/csrc/quant_remap.h, the function the kernel calls), run on the host
under UBSan over the extreme ids that never go near a GPU: ``INT64_MIN``,
``INT64_MAX``, ``2**40``, and the edges ``-1``, ``0``, ``rows - 1``, ``rows``,
with and without a remap.

A stand-alone C++ program with its own ``main`` includes the header, is built
with the host compiler and ``-fsanitize=undefined -fno-sanitize-recover=all``
(any signed overflow or out-of-bounds index in the decision aborts it), and
checks every result itself. Nothing is preloaded and no Python extension is
loaded."""

import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "torchrec_amd", "ops", "csrc"
)

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <limits>

#include "quant_remap.h"

using trec_amd::quant_remap_id;

static int failures = 0;

static void expect(int64_t idx, int64_t rows, const int32_t* remap, int64_t want_row,
                   bool want_oob) {
  bool oob = !want_oob;
  int64_t got = quant_remap_id(idx, rows, remap, &oob);
  if (got != want_row || oob != want_oob) {
    std::printf("FAIL idx=%lld rows=%lld remap=%d: got (%lld, %d), want (%lld, %d)\n",
                (long long)idx, (long long)rows, remap != nullptr, (long long)got, (int)oob,
                (long long)want_row, (int)want_oob);
    ++failures;
  }
}

int main() {
  const int64_t kMin = std::numeric_limits<int64_t>::min();
  const int64_t kMax = std::numeric_limits<int64_t>::max();
  const int64_t kBig = int64_t(1) << 40;
  // exactly `rows` entries: UBSan's bounds check sees an index past them
  static const int32_t remap[6] = {3, -1, 0, -1, 1, 2};
  const int64_t rows = 6;
  const int64_t dropped[] = {kMin, kMin + 1, -2, -1, rows, rows + 1, kBig, kMax - 1, kMax};
  for (int64_t idx : dropped) {
    expect(idx, rows, nullptr, -1, true);
    expect(idx, rows, remap, -1, true);
    expect(idx, 0, nullptr, -1, true);  // an empty table keeps nothing
  }
  expect(0, 0, nullptr, -1, true);
  for (int64_t idx = 0; idx < rows; ++idx) {
    expect(idx, rows, nullptr, idx, false);
    expect(idx, rows, remap, remap[idx], false);  // -1 for a pruned id, not out of range
  }
  expect(0, rows, remap, 3, false);
  expect(1, rows, remap, -1, false);
  expect(rows - 1, rows, remap, 2, false);
  // a table with more ids than int32: no remap, ids near 2**40 are in range
  expect(kBig, kBig + 1, nullptr, kBig, false);
  expect(kBig + 1, kBig + 1, nullptr, -1, true);
  expect(kMax - 1, kMax, nullptr, kMax - 1, false);
  expect(kMax, kMax, nullptr, -1, true);
  expect(kMin, kMax, nullptr, -1, true);
  if (failures == 0) std::printf("OK\n");
  return failures == 0 ? 0 : 1;
}
"""


def host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.mark.skipif(host_compiler() is None, reason="no host C++ compiler")
def test_remap_decision_under_ubsan(tmp_path):
    src = tmp_path / "remap_host.cpp"
    exe = tmp_path / "remap_host"
    src.write_text(PROGRAM)
    build = subprocess.run(
        [host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=undefined",
         "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
        capture_output=True, text=True,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "OK" and "runtime error" not in run.stderr
