"""A generated kernel's cache key is its shape spec (hr_rtc_gen.hpp: RtcSpec), and the spec is all its generator reads.
tools/rtc_check.cpp, built with -DRTC_SOURCES_ONLY against hr_rtc_gen.hip alone — the generator is pure host code and links
without the library, hiprtc or a GPU —, perturbs every input of every maker over its whole matrix of shapes, one field at a
time (tools/rtc_shapes.hpp): a source that changes must change the spec, and a spec that changes must change the source
except where the header lists why not."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not on PATH")
def test_specs_and_sources_change_together(tmp_path):
    algo = os.path.join(ROOT, "aresdb_amd", "csrc", "algo")
    exe = tmp_path / "rtc_sources"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-DRTC_SOURCES_ONLY", "-I" + os.path.join(ROOT, "include"),
                    "-I" + algo, "-o", str(exe), os.path.join(ROOT, "tools", "rtc_check.cpp"), os.path.join(algo, "hr_rtc_gen.hip")],
                   check=True, timeout=600)
    out = subprocess.run([str(exe), str(tmp_path / "k")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    m = re.search(r"spec versus source: (\d+) shapes, (\d+) perturbations, (\d+) violations", out.stdout)
    assert m, out.stdout[-2000:]
    shapes, pairs, bad = (int(g) for g in m.groups())
    assert bad == 0 and shapes >= 50 and pairs >= 3000, m.group(0)
    assert "WRONG KERNEL" not in out.stdout and "over-specified" not in out.stdout
    # every shape's source was written, and is text
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hip")]) >= 48
