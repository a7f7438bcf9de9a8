"""The Sort + Reduce scan (hr_rtc.hip, SCAN_SORT64) generated for AVG_FLOAT — the record carries the float the measure transform
would have stored and, in the top bit of its row word, "null measure" — compiles for gfx950 without a GPU
(tools/rtc_check_avg.cpp) for the C3 and the trips shape, stays within 128 VGPRs without scratch, and costs a handful of vector
instructions more than the SUM_FLOAT-into-float64 scan of the same shape, generated and compiled in the same run.

Measured (static count of v_ instructions in the code object, ROCm 7 hiprtc, -O3): C3 965 -> 992, trips 731 -> 758: + 27 = four
rows x (three for the bit: xor, and, shift-or into `alive`; two for the row word: and, or) + a few moves around them.  The
budget is + 32 (four rows x eight), the way the float expression's budget of tests/test_rtc_float_sort_sources.py is its
sibling's + 8; the C3 scan also stays inside that file's absolute budget (1015) + 32.  The integer conversions (to double, then
to float: two instructions a row) ride on top: + 8 more."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _facts(co):
    notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True)
    dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True)
    if notes.returncode != 0 or dis.returncode != 0 or ".vgpr_count" not in notes.stdout:
        return None  # (tools absent: the compile check still holds)
    return {"scratch": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes.stdout).group(1)),
            "vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", notes.stdout).group(1)),
            "lds": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes.stdout).group(1)),
            "valu": sum(1 for ln in dis.stdout.splitlines() if ln.strip().startswith("v_"))}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_average_sort_scans_compile_beside_their_float_sum_siblings(tmp_path):
    lib = os.path.join(ROOT, "aresdb_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libalgorithm.so")):
        pytest.skip("libalgorithm.so not built")
    exe = tmp_path / "rtc_check_avg"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "aresdb_amd", "csrc", "algo"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "rtc_check_avg.cpp"), "-L" + lib, "-lalgorithm", "-lhiprtc", "-Wl,-rpath," + lib],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp_path / "k")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]  # (non-zero: a compile failed, or a plan was not declined)
    for what in ("C3 sort scan (AVG_FLOAT)", "trips sort scan (AVG_FLOAT)", "C3 sort scan (AVG of an Int32 column)",
                 "C3 sort scan (AVG of a Uint32 column + 5)", "C3 sort scan (AVG into an Int64-typed measure)", "C3 sort scan (AVG of m * 1.5)"):
        assert f"{what} compile rc 0" in out.stdout, what
    src = (tmp_path / "k_c3_avg.hip").read_text()
    assert "alive[j] |= (alive[j] & (okb ^ 1u)) << 31;" in src and "(a.rowBase + i0 + j) | (alive[j] & 0x80000000u)" in src
    assert "(float)(double)(i32)x" in (tmp_path / "k_c3_avg_i32.hip").read_text()
    facts = {tag: _facts(str(tmp_path / f"k_{tag}.co")) for tag in
             ("c3_fsum8", "c3_avg", "trips_fsum8", "trips_avg", "c3_avg_i32", "c3_avg_u32", "c3_avg_u32_i64", "c3_avg_fexpr")}
    if any(f is None for f in facts.values()):
        return
    print({tag: f["valu"] for tag, f in facts.items()})
    for tag, f in facts.items():
        assert f["scratch"] == 0 and f["vgprs"] <= 128 and f["lds"] <= 160 * 1024, (tag, f)
    for shape in ("c3", "trips"):
        extra = facts[shape + "_avg"]["valu"] - facts[shape + "_fsum8"]["valu"]
        assert extra <= 32, (shape, extra)
    assert facts["c3_avg"]["valu"] <= 1015 + 32, facts["c3_avg"]
    for tag in ("c3_avg_i32", "c3_avg_u32", "c3_avg_u32_i64"):
        assert facts[tag]["valu"] - facts["c3_fsum8"]["valu"] <= 32 + 8, (tag, facts[tag])
    assert facts["c3_avg_fexpr"]["valu"] - facts["c3_fsum8"]["valu"] <= 32 + 8, facts["c3_avg_fexpr"]  # (+ 4 multiplies, 4 selects)
