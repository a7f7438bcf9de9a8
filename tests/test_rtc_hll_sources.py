"""HyperLogLog's pre-aggregation scan (hr_rtc.hip: generate_vector, hll) checked without a GPU, the way
test_rtc_wide_sources.py checks the vector-sourced sort scans: tools/rtc_check.cpp asks the library for the sources and hands
them to hiprtc for gfx950; the code objects' notes give registers, LDS and scratch; the statements that compute the key are
compiled for the host and compared with the oracle's murmur3_x64_128 of the packed row."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# tag of the code object -> (what rtc_check prints, slot widths, scratch allowed: the eight-dimension shape shares the
# footprint of the sort scan's — 128 VGPRs and a few bytes of scratch per lane —, every other shape stays in registers)
HLL = {
    "k_hll1": ("hll scan, slot 4", (4,), False),
    "k_hll_narrow": ("hll scan, slots 4 4 2 1", (4, 4, 2, 1), False),
    "k_hll8": ("hll scan nd 8", (4,) * 8, True),
    "k_hll_16_4": ("hll scan, slots 16 4", (16, 4), False),
    "k_hll_16_8_4_4": ("hll scan, slots 16 8 4 4", (16, 8, 4, 4), False),
}


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    lib = os.path.join(ROOT, "aresdb_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libalgorithm.so")):
        pytest.skip("libalgorithm.so not built")
    tmp = tmp_path_factory.mktemp("rtc_hll")
    exe = tmp / "rtc_check"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "aresdb_amd", "csrc", "algo"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "rtc_check.cpp"), "-L" + lib, "-lalgorithm", "-lhiprtc", "-Wl,-rpath," + lib],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp / "k")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return tmp, out.stdout


def test_hll_scans_compile_for_gfx950(checked):
    _, stdout = checked
    for what, _, _ in HLL.values():
        assert f"{what} compile rc 0" in stdout, what


@pytest.mark.parametrize("tag", sorted(HLL))
def test_hll_scans_fit_a_1024_lane_workgroup(checked, tag):
    """1024 lanes = four wavefronts per SIMD: at most 128 VGPRs; one workgroup per CU: LDS within 160 KB; no scratch."""
    tmp, _ = checked
    _, _, scratch_allowed = HLL[tag]
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp / f"{tag}.co")], capture_output=True, text=True)
    if notes.returncode != 0 or ".vgpr_count" not in notes.stdout:
        pytest.skip("llvm-readelf not available")
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", notes.stdout).group(1))
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes.stdout).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes.stdout).group(1))
    assert vgprs <= 128 and lds <= 160 * 1024, (tag, vgprs, lds)
    assert scratch <= (16 if scratch_allowed else 0), (tag, scratch)
    assert "hll_scan_rtc" in notes.stdout


def test_the_partition_is_a_scramble_of_the_whole_key(checked):
    """All registers of one dimension row share the key's upper 48 bits: the partition must not be the key's top bits."""
    tmp, _ = checked
    src = (tmp / "k_hll_narrow.hip").read_text()
    assert "#define PB 9" in src and "hll_scan_rtc" in src
    assert "(hh[j] ^ (cw[j] * 0x9E3779B1u)) * 0x85EBCA6Bu" in src
    # ... and it spreads 16384 registers of one row evenly over the 512 partitions
    hh = np.uint32(0x1234ABCD)
    cw = (np.uint32(0xBEEF0000) | np.arange(1 << 14, dtype=np.uint32))
    part = ((hh ^ (cw * np.uint32(0x9E3779B1))) * np.uint32(0x85EBCA6B)) >> np.uint32(23)
    counts = np.bincount(part.astype(np.int64), minlength=512)
    assert counts.min() >= 16 and counts.max() <= 64, (counts.min(), counts.max())


_HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
typedef unsigned int u32; typedef unsigned long long u64; typedef unsigned char u8;
#define __device__
#define __forceinline__ inline
%(prelude)s
struct Raw { u32 v[%(nw)d][4]; u32 ok[%(nd)d]; u32 m[4]; };
int main() {
  Raw r;
  for (;;) {
    memset(&r, 0, sizeof(r));
    for (int j = 0; j < 4; j++) {
      for (int w = 0; w < %(nw)d; w++) if (scanf("%%u", &r.v[w][j]) != 1) return 0;
      for (int d = 0; d < %(nd)d; d++) { u32 ok; if (scanf("%%u", &ok) != 1) return 0; r.ok[d] |= ok << (8 * j); }
      if (scanf("%%u", &r.m[j]) != 1) return 0;
    }
    for (int j = 0; j < 4; j++) {
      u64 h64;
%(block)s
      printf("%%llu\n", h64);
    }
  }
}
"""


@pytest.mark.parametrize("tag", ["k_hll1", "k_hll_narrow", "k_hll8", "k_hll_16_8_4_4"])
def test_generated_key_is_the_oracles(checked, tag):
    """key = (lo64(murmur3_x64_128(packed row)) & ~0xFFFF) | (hll value & 0x3FFF) — the row packed as [values, widest
    first][one validity byte per dimension] and hashed by the oracle; seeded rows, hll values with bits 14-15 set among them."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    oracle_so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    if not os.path.exists(oracle_so):
        pytest.skip("oracle not built")
    tmp, _ = checked
    widths = HLL[tag][1]
    src = (tmp / f"{tag}.hip").read_text().splitlines()
    prelude = "\n".join(ln for ln in src if ln.startswith("#define MC") or "rotl64(u64 x" in ln or "fmix64(u64 k)" in ln)
    first = next(i for i, ln in enumerate(src) if ln.strip() == "u64 h64;")
    last = next(i for i, ln in enumerate(src) if ln.strip().startswith("hh[j] = (u32)(h64 >> 32)"))
    block = src[first + 1:last]
    assert any("0xFFFFFFFFFFFF0000ull" in ln and "0x3FFFu" in ln for ln in block), block[-3:]
    nd, nw = len(widths), sum(max(1, w // 4) for w in widths)
    main = tmp / f"{tag}_host.cpp"
    main.write_text(_HOST_MAIN % {"prelude": prelude, "nw": nw, "nd": nd, "block": "\n".join(block)})
    exe = tmp / f"{tag}_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(main)], check=True, timeout=300)
    rng = np.random.default_rng(len(tag))
    n = 64
    words = rng.integers(0, 1 << 32, (n, nw), dtype=np.uint64).astype(np.uint32)
    words[0] = 0
    words[1] = 0xFFFFFFFF
    # a slot narrower than four bytes holds its value zero-extended in its word
    col = 0
    for w in widths:
        k = max(1, w // 4)
        if w < 4:
            words[:, col] &= (1 << (8 * w)) - 1
        col += k
    valid = (rng.random((n, nd)) > 0.2).astype(np.uint32)
    hll = ((rng.integers(0, 52, n) << 16) | (rng.integers(0, 4, n) << 14) | rng.integers(0, 1 << 14, n)).astype(np.uint32)
    text = "\n".join(" ".join(map(str, list(words[i]) + list(valid[i]) + [hll[i]])) for i in range(n)) + "\n"
    got = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert got.returncode == 0, got.stderr
    got = [int(x) for x in got.stdout.split()]
    lib = ctypes.CDLL(oracle_so)
    lib.oracle_murmur3_128.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    h = (ctypes.c_uint64 * 2)()
    want = []
    for i in range(n):
        row, col = b"", 0
        for w in widths:
            k = max(1, w // 4)
            row += words[i, col:col + k].tobytes()[:w]
            col += k
        row += bytes(int(v) for v in valid[i])
        lib.oracle_murmur3_128(row, len(row), 0, h)
        want.append((h[0] & 0xFFFFFFFFFFFF0000) | (int(hll[i]) & 0x3FFF))
    assert got == want
