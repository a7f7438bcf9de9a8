"""The scans and the merge generated for constant-chain time dimensions (tools/rtc_check_chain.cpp: the trips shape grouped by
[chain, city_id]) compile for gfx950 without a GPU, hold no private segment, stay within 128 VGPRs and within their chain-free
sibling's LDS, and cost what their steps cost — the scans are bound by vector-ALU issue, so an instruction count is a speed.
The budget is derived from the same run: a division-like step costs what Floor(request_at, 3600) costs over the bare column in
the chain-free siblings, a Plus / Minus step one instruction for each of a lane's four elements.  A float chain and a
null-constant chain are declined: rtc_check_chain returns an error if the generator answers them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"

# chain -> (Plus / Minus steps, division-like steps) in front of its division-like root, whose own cost the Floor sibling holds
CHAINS = {"zone_hour": (1, 0), "hour_of_day": (0, 1), "zone_time_of_day": (1, 0), "hour_of_week": (1, 1), "zone_hour_of_week": (2, 1)}
KINDS = ("lines16", "compact", "table", "sort64", "merge")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_chain_kernels_compile_within_their_siblings_budgets(tmp_path):
    lib = os.path.join(ROOT, "aresdb_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libalgorithm.so")):
        pytest.skip("libalgorithm.so not built")
    exe = tmp_path / "rtc_check_chain"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "aresdb_amd", "csrc", "algo"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "rtc_check_chain.cpp"), "-L" + lib, "-lalgorithm", "-lhiprtc", "-Wl,-rpath," + lib],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp_path / "k")], capture_output=True, text=True, timeout=900)
    # (a nonzero status also covers: the offset is text, a divisor is not, a declined chain answered, a source off its spec)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    for tag in ("bare", "floor", *CHAINS):
        for kind in KINDS:
            what = f"{tag} {kind} scan" if kind != "merge" else f"{tag} merge"
            assert f"{what} compile rc 0" in out.stdout, what
    # the offset travels as an argument, the null row is zeroed once, behind the root
    src = (tmp_path / "k_zone_hour_compact.hip").read_text()
    assert re.search(r"ch = ch \+ a\.k\[\d+\];", src) and "0xffff8f80u" not in src.lower()
    assert "-28800" not in src

    def stats(tag, kind):
        co = str(tmp_path / f"k_{tag}_{kind}.co")
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True)
        dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True)
        if notes.returncode != 0 or dis.returncode != 0 or ".vgpr_count" not in notes.stdout:
            return None  # (tools absent: the compile check above still holds)
        return {"private": ".private_segment_fixed_size: 0" in notes.stdout,
                "vgprs": int(re.search(r"\.vgpr_count:\s+(\d+)", notes.stdout).group(1)),
                "lds": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes.stdout).group(1)),
                "valu": sum(1 for ln in dis.stdout.splitlines() if ln.strip().startswith("v_"))}
    for kind in KINDS:
        bare, floor = stats("bare", kind), stats("floor", kind)
        if bare is None or floor is None:
            continue
        division = floor["valu"] - bare["valu"]  # what one division-like step costs in this kernel
        assert division > 0, (kind, bare, floor)
        for tag, (adds, divisions) in CHAINS.items():
            s = stats(tag, kind)
            limit = floor["valu"] + 4 * adds + division * divisions + 8
            print(f"{tag} {kind}: VALU {s['valu']} (limit {limit}: sibling {floor['valu']}, a division {division}), VGPRs {s['vgprs']}, LDS {s['lds']}")
            assert s["private"], (tag, kind)
            assert s["vgprs"] <= 128 and s["lds"] <= floor["lds"], (tag, kind, s)
            assert s["valu"] <= limit, (tag, kind, s["valu"], limit)
