"""The Sort + Reduce scan (hr_rtc.hip, SCAN_SORT64) generated for FLOAT measures — SUM of a Float32 column into float64 (the
headline query under the reference's shipped configuration), MIN_FLOAT into 4 bytes, SUM(m * 1.5) — compiles for gfx950 without
a GPU (tools/rtc_check.cpp) and stays inside the budgets of its integer sibling of the same shape (k_sort_sum8 of
tests/test_rtc_sources.py): the scans are bound by vector-ALU issue, so an instruction count is a speed.  Shapes a record cannot
carry (a float column times an integer constant, an integer column into a 4-byte float measure) are declined: rtc_check
returns an error if the generator answers them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_float_measure_sort_scans_compile_within_the_integer_budgets(tmp_path):
    lib = os.path.join(ROOT, "aresdb_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libalgorithm.so")):
        pytest.skip("libalgorithm.so not built")
    exe = tmp_path / "rtc_check"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "aresdb_amd", "csrc", "algo"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "rtc_check.cpp"), "-L" + lib, "-lalgorithm", "-lhiprtc", "-Wl,-rpath," + lib],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp_path / "k")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for what in ("sort scan (SUM_FLOAT into 8 bytes)", "sort scan (MIN_FLOAT)", "sort scan (float expression)"):
        assert f"{what} compile rc 0" in out.stdout, what
    # the float product is one multiply on the measure's bits, rounded once: no conversion, no fused multiply-add
    src = (tmp_path / "k_sort_fexpr.hip").read_text()
    assert "__uint_as_float(v) * __uint_as_float(a.k[" in src
    for tag, limit in {"k_sort_fsum8": 1015, "k_sort_fmin": 1015, "k_sort_fexpr": 1015 + 8}.items():  # (+ 4 multiplies, 4 selects)
        co = str(tmp_path / f"{tag}.co")
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True)
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True)
        if notes.returncode != 0 or dis.returncode != 0 or ".vgpr_count" not in notes.stdout:
            continue  # (tools absent: the compile check above still holds)
        assert ".private_segment_fixed_size: 0" in notes.stdout, tag
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", notes.stdout).group(1))
        lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes.stdout).group(1))
        assert vgprs <= 128 and lds <= 160 * 1024, (tag, vgprs, lds)
        valu = sum(1 for ln in dis.stdout.splitlines() if ln.strip().startswith("v_"))
        assert valu <= limit, (tag, valu, limit)
        if tag == "k_sort_fexpr":
            assert "v_mul_f32" in dis.stdout and "v_fma_f32" not in dis.stdout and "v_fmac_f32" not in dis.stdout
