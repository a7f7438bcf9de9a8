"""The vector-sourced sort scan (hr_rtc.hip: generate_vector, sort64) over dimension slots of 8 and 16 bytes — Int64 /
Uint64 / GeoPoint and UUID group keys on the Sort + Reduce path — checked without a GPU, the way test_rtc_sources.py checks
the other generated kernels: tools/rtc_check.cpp asks the library for the sources and hands them to hiprtc for gfx950; the
code objects' notes and disassembly give registers, LDS, scratch and the vector-instruction count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# tag of the code object -> (what rtc_check prints, value bytes per row, vector-instruction budget = the count when the shape
# was added + ~5 %: the scan is bound by vector-ALU issue, so a count that creeps up is a slowdown no test of results sees)
WIDE = {
    "k_vsort_16_4": ("vector sort scan, slots 16 4", 20, 1075),
    "k_vsort_8_8_4_4": ("vector sort scan, slots 8 8 4 4", 24, 1190),
    "k_vsort_16_8_4_4": ("vector sort scan, slots 16 8 4 4", 32, 1365),
    "k_vsort_8_4_2_1": ("vector sort scan, slots 8 4 2 1", 15, 1190),
    "k_vsort_8": ("vector sort scan, slot 8, one partition", 8, 700),
}


@pytest.fixture(scope="module")
def checked(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    lib = os.path.join(ROOT, "aresdb_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libalgorithm.so")):
        pytest.skip("libalgorithm.so not built")
    tmp = tmp_path_factory.mktemp("rtc_wide")
    exe = tmp / "rtc_check"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "aresdb_amd", "csrc", "algo"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "rtc_check.cpp"), "-L" + lib, "-lalgorithm", "-lhiprtc", "-Wl,-rpath," + lib],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp / "k")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return tmp, out.stdout


def test_wide_slot_scans_compile_for_gfx950(checked):
    _, stdout = checked
    for tag, (what, _, _) in WIDE.items():
        assert f"{what} compile rc 0" in stdout, what


@pytest.mark.parametrize("tag", sorted(WIDE))
def test_wide_slot_scans_fit_a_1024_lane_workgroup(checked, tag):
    """1024 lanes = four wavefronts per SIMD: at most 128 VGPRs; one workgroup per CU: LDS within 160 KB.  Rows of up to 24
    value bytes keep their working set in registers (no scratch); the 32-byte row is held to the register and LDS limits like
    the eight-dimension shape (k_vsort8 of test_rtc_sources.py) whose footprint it shares."""
    tmp, _ = checked
    _, value_bytes, limit = WIDE[tag]
    co = str(tmp / f"{tag}.co")
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], capture_output=True, text=True)
    if notes.returncode != 0 or dis.returncode != 0 or ".vgpr_count" not in notes.stdout:
        pytest.skip("llvm-readelf / llvm-objdump not available")
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", notes.stdout).group(1))
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes.stdout).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes.stdout).group(1))
    assert vgprs <= 128 and lds <= 160 * 1024, (tag, vgprs, lds)
    if value_bytes <= 24:
        assert scratch == 0, (tag, scratch)
    valu = sum(1 for ln in dis.stdout.splitlines() if ln.strip().startswith("v_"))
    assert valu <= limit, (tag, valu, limit)


def test_wide_slot_scan_reads_whole_quads(checked):
    """Four rows of an 8-byte slot are two 16-byte loads, of a 16-byte slot four: no narrower load of a wide slot's values in
    the full-tile path (the tail reads words)."""
    tmp, _ = checked
    src = (tmp / "k_vsort_16_8_4_4.hip").read_text()
    full = src[src.index("void load_full"):src.index("void load_tail")]
    assert full.count("const PU32x4 t") >= 4 + 2 + 1 + 1, full
    assert "#define NW 8" in src



_HOST_MAIN = r"""
#include <cstdio>
#include <cstring>
typedef unsigned int u32; typedef unsigned long long u64; typedef unsigned char u8;
#define __device__
#define __forceinline__ inline
%(prelude)s
struct Raw { u32 v[%(nw)d][4]; u32 ok[%(nd)d]; };
int main() {
  Raw r;
  for (;;) {
    memset(&r, 0, sizeof(r));
    for (int j = 0; j < 4; j++) {
      for (int w = 0; w < %(nw)d; w++) if (scanf("%%u", &r.v[w][j]) != 1) return 0;
      for (int d = 0; d < %(nd)d; d++) { u32 ok; if (scanf("%%u", &ok) != 1) return 0; r.ok[d] |= ok << (8 * j); }
    }
    for (int j = 0; j < 4; j++) {
      u64 h64;
%(block)s
      printf("%%llu\n", h64);
    }
  }
}
"""


@pytest.mark.parametrize("tag,widths", [("k_vsort_16_8_4_4", (16, 8, 4, 4)), ("k_vsort_8_4_2_1", (8, 4, 2, 1)), ("k_vsort_16_4", (16, 4)),
                                        ("k_vsort_8", (8,))])
def test_generated_hash_of_a_wide_row_is_the_oracles_murmur(checked, tag, widths):
    """The statements the generator writes for the 64-bit row hash, compiled for the host and run on fixed and random rows,
    against murmur3_x64_128 of the packed row [values, widest first][one validity byte per dimension] as the oracle computes
    it — what the real Sort orders by."""
    import ctypes
    import numpy as np
    if shutil.which("g++") is None:
        pytest.skip("g++ not on PATH")
    oracle_so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    if not os.path.exists(oracle_so):
        pytest.skip("oracle not built")
    tmp, _ = checked
    src = (tmp / f"{tag}.hip").read_text().splitlines()
    prelude = "\n".join(ln for ln in src if ln.startswith("#define MC") or "rotl64(u64 x" in ln or "fmix64(u64 k)" in ln)
    first = next(i for i, ln in enumerate(src) if ln.strip() == "u64 h64;")
    last = next(i for i, ln in enumerate(src) if ln.strip().startswith("hh[j] = (u32)(h64 >> 32)"))
    nd, nw = len(widths), sum(max(1, w // 4) for w in widths)
    main = tmp / f"{tag}_host.cpp"
    main.write_text(_HOST_MAIN % {"prelude": prelude, "nw": nw, "nd": nd, "block": "\n".join(src[first + 1:last])})
    exe = tmp / f"{tag}_host"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), str(main)], check=True, timeout=300)
    rng = np.random.default_rng(len(tag))
    n = 64
    words = rng.integers(0, 1 << 32, (n, nw), dtype=np.uint64).astype(np.uint32)
    words[0] = 0
    words[1] = 0xFFFFFFFF
    words[2] = words[3]
    words[2, 0] ^= 1            # rows that differ in one word only: the first ...
    words[4] = words[5]
    words[4, nw - 1] ^= 0x80000000  # ... and the last
    valid = (rng.random((n, nd)) >= 0.2).astype(np.uint32)
    at = 0
    for w in widths:  # a narrow slot's word is its value, zero-extended
        if w < 4:
            words[:, at] &= (1 << (8 * w)) - 1
        at += max(1, w // 4)
    text = "\n".join(" ".join(map(str, list(words[i]) + list(valid[i]))) for i in range(n))
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60, check=True)
    got = [int(x) for x in out.stdout.split()]
    lib = ctypes.CDLL(oracle_so)
    lib.oracle_murmur3_128.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    h = (ctypes.c_uint64 * 2)()
    want = []
    for i in range(n):
        row, at = b"", 0
        for w in widths:
            k = max(1, w // 4)
            row += words[i, at:at + k].tobytes()[:w]
            at += k
        row += bytes(int(v) for v in valid[i])
        lib.oracle_murmur3_128(row, len(row), 0, h)
        want.append(int(h[0]))
    assert got == want
    assert len(set(got[2:6])) == 4
