"""The structs of AresFusedFilterJoinSelect: aresdb_amd/abi.py's ctypes mirrors against what a C compiler makes of
include/ares_extensions.h, and the two entry points among libalgorithm.so's exports.  No GPU needed (nothing is called)."""
import ctypes as C
import os
import subprocess

import test_abi_exports as X
from aresdb_amd import abi

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ares_extensions.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m))
int main(void) {
  printf("AresFusedJoin %zu\nAresFusedJoinSelect %zu\n", sizeof(AresFusedJoin), sizeof(AresFusedJoinSelect));
  F(AresFusedJoin, key); F(AresFusedJoin, index);
  F(AresFusedJoinSelect, numFilters); F(AresFusedJoinSelect, filters); F(AresFusedJoinSelect, numJoins); F(AresFusedJoinSelect, joins);
  F(AresFusedJoinSelect, numForeignFilters); F(AresFusedJoinSelect, foreignFilters); F(AresFusedJoinSelect, foreignFilterJoin);
  F(AresFusedJoinSelect, numDims); F(AresFusedJoinSelect, dims); F(AresFusedJoinSelect, dimJoin);
  return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(PROGRAM)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(abi.REPO_ROOT, "include"), str(src), "-o", str(exe)])
    seen = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    mirrors = {"AresFusedJoin": abi.FusedJoin, "AresFusedJoinSelect": abi.FusedJoinSelect}
    assert len(seen) == 14
    for name, value in seen.items():
        struct, _, member = name.partition(".")
        want = getattr(mirrors[struct], member).offset if member else C.sizeof(mirrors[struct])
        assert int(value) == want, name
    for struct in mirrors.values():
        assert {"AresFused" + struct.__name__[5:] + "." + f[0] for f in struct._fields_} <= set(seen)


def test_libalgorithm_exports_the_entry_points():
    algo, _ = X._built()
    lib = C.CDLL(algo, mode=os.RTLD_NOW | os.RTLD_LOCAL)
    for name in ("AresFusedFilterJoinSelect", "AresSelectJoinStats"):
        assert getattr(lib, name) is not None
