"""Scratch frames DEFINED as constant chains (deferral.hpp: FrameDef), through the ABI directly: every exit of a definition.
A frame that somebody reads — a copy, a node that does not compose, a fallback that launches the queue — holds exactly what the
node-by-node sequence leaves in it (the oracle's bytes); a frame nobody reads is never written: overwritten by its own next
node, freed, its stream destroyed.  The kernel log says which: transform_fast_kernel runs only where a reader existed.
A seeded random interleaving of the same steps is compared, read by read, with the oracle and with an ARES_DEFER=0 process."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_model as M
import harness as H
from aresdb_amd import abi

N = 4099 + 1024  # more than one workgroup tile, odd
OFF = -28800


def _on():
    return all(os.environ.get(k, "1") != "0" for k in ("ARES_FUSE", "ARES_DEFER", "ARES_CHAINS"))


class World:
    """One batch's buffers on one backend: the time column (3 % nulls, the edge timestamps first), an index vector, three
    scratch frames, a one-dimension vector pair and a measure vector."""

    def __init__(self, be, n=N, seed=1, stream=None):
        rng = np.random.default_rng(seed)
        self.be, self.n, self.size, self.stream = be, n, n, stream
        ts = (2 * 86400 + rng.integers(0, 10 * 86400, n)).astype(np.uint32)
        ts[:len(M.EDGE_TS)] = M.EDGE_TS
        self.ts_values, self.ts_valid = ts, rng.random(n) >= 0.03
        self.col = H.Column(be, abi.Uint32, ts, valid=self.ts_valid)
        self.fare = H.Column(be, abi.Float32, (rng.integers(0, 400, n) / 4).astype(np.float32))
        self.idx = H.Buf(be, nbytes=4 * n)
        self.pred = H.Buf(be, nbytes=n)
        self.frames = {k: H.Scratch(be, n, abi.Int32) for k in "ABC"}
        self.dims = [H.DimVector(be, n, (0, 0, 1, 0, 0)) for _ in range(2)]
        self.meas = [H.Buf(be, nbytes=8 * n) for _ in range(2)]
        be.call("InitIndexVector", self.idx.ptr, 0, n, stream, 0)

    # -- the calls ---------------------------------------------------------------------------------------------------------
    def filter(self, functor, const):
        self.size = self.be.call("BinaryFilter", self.col.input(), H.const_int(const), self.idx.ptr, self.pred.ptr, self.size, None, 0, None,
                                 0, functor, self.stream, 0)

    def node(self, functor, lhs, const, out):
        """frame `out` = (column | frame `lhs`) functor const"""
        a = self.col.input() if lhs == "ts" else self.frames[lhs].input()
        self.be.call("BinaryTransform", a, H.const_int(const), self.frames[out].output(), self.idx.ptr, self.size, None, 0, functor,
                     self.stream, 0)

    def two_columns(self, functor, lhs, rhs, out):
        self.be.call("BinaryTransform", self.frames[lhs].input(), self.frames[rhs].input(), self.frames[out].output(), self.idx.ptr, self.size,
                     None, 0, functor, self.stream, 0)

    def root(self, functor, lhs, const):
        """dimension rows [0, size) = frame `lhs` functor const"""
        vo, no, _ = self.dims[0].dim_offsets()[0]
        a = self.col.input() if lhs == "ts" else self.frames[lhs].input()
        self.be.call("BinaryTransform", a, H.const_int(const), H.dimension_output(self.dims[0].values.ptr + vo, self.dims[0].values.ptr + no, abi.Uint32),
                     self.idx.ptr, self.size, None, 0, functor, self.stream, 0)

    def measure(self):
        self.be.call("UnaryTransform", self.fare.input(), H.measure_output(self.meas[0].ptr, abi.Float64, abi.AGGR_SUM_FLOAT), self.idx.ptr,
                     self.size, None, 0, abi.Noop, self.stream, 0)

    def hash_reduce(self):
        g = self.be.call("HashReduce", self.dims[0].struct(), self.meas[0].ptr, self.dims[1].struct(), self.meas[1].ptr, 8, self.size,
                         abi.AGGR_SUM_FLOAT, self.stream, 0)
        self.be.wait(self.stream)
        rows = self.dims[1].rows(g)
        return dict(zip(rows, self.meas[1].read(np.float64, g).tolist()))

    def rewrite_column(self, seed):
        """the host writes new timestamps into the column (a copy through libmem)"""
        rng = np.random.default_rng(seed)
        self.ts_values = (86400 + rng.integers(0, 20 * 86400, self.n)).astype(np.uint32)
        vp = self.col.vp
        H.upload(self.be, vp.BasePtr + vp.ValuesOffset, self.ts_values)

    def replace_frame(self, k):
        self.frames[k].free()
        self.frames[k] = H.Scratch(self.be, self.n, abi.Int32)

    # -- the reads ---------------------------------------------------------------------------------------------------------
    def read_frame(self, k):
        f = self.frames[k]
        return f.values()[:self.size].tobytes() + f.valid()[:self.size].tobytes()

    def read_dim(self):
        vo, no, _ = self.dims[0].dim_offsets()[0]
        blob = self.dims[0].values.read(np.uint8)
        return blob[vo:vo + 4 * self.size].tobytes() + blob[no:no + self.size].tobytes()

    def free(self):
        for x in [self.col, self.fare, self.idx, self.pred, *self.frames.values(), *self.dims, *self.meas]:
            x.free()


def both(program, seed=1):
    """runs `program(world)` (it returns what it read) on the hip backend under the kernel log and on the oracle"""
    hip, oracle = H.hip_backend(), H.oracle_backend()
    wo = World(oracle, seed=seed)
    want = program(wo)
    wo.free()
    wh = World(hip, seed=seed)
    hip.wait()
    hip.profiler_enable(True)
    try:
        got = program(wh)
        hip.wait()
        kernels = hip.profiler_report()
    finally:
        hip.profiler_enable(False)
    wh.free()
    return got, want, kernels


def launches(kernels, prefix="transform"):
    return {k: v[0] for k, v in kernels.items() if k.startswith(prefix)}


@pytest.mark.gpu
def test_copy_of_the_frame_before_the_root_call():
    def program(w):
        w.node(abi.Plus, "ts", OFF, "A")
        a = w.read_frame("A")  # the reader: the frame is written now
        w.root(abi.Floor, "A", 3600)  # (the frame exists: the root reads it like any scratch operand)
        return a, w.read_dim()
    got, want, kernels = both(program)
    assert got == want
    if _on():
        assert launches(kernels).get("transform_fast_kernel") == 1 and "transform32_kernel" in kernels, kernels


@pytest.mark.gpu
def test_copy_of_the_frame_after_the_root_call():
    def program(w):
        w.node(abi.Plus, "ts", OFF, "A")
        w.node(abi.Mod, "A", 86400, "B")
        w.root(abi.Floor, "B", 3600)  # composed: a queued job over the column
        return w.read_frame("B"), w.read_frame("A"), w.read_dim()
    got, want, kernels = both(program)
    assert got == want
    if _on():  # B, A and the queued job: one launch each, all of them chains over the column
        assert launches(kernels) == {"transform_fast_kernel": 3}, kernels


@pytest.mark.gpu
def test_a_frame_nobody_reads_is_never_written():
    def program(w):
        w.filter(abi.GreaterThanOrEqual, 3600)
        w.node(abi.Plus, "ts", OFF, "A")
        w.node(abi.Minus, "A", 345600, "A")  # the frame overwritten by its own next node
        w.node(abi.Mod, "A", 604800, "B")
        w.root(abi.Floor, "B", 3600)
        w.be.wait(w.stream)
        w.replace_frame("A")  # freed
        w.replace_frame("B")
        before = dict(w.be.profiler_report()) if w.be.name == "hip" else {}
        return w.read_dim(), before
    got, want, kernels = both(program)
    assert got[0] == want[0]
    if _on():
        assert not launches(got[1]), got[1]  # nothing until the dimension rows were read ...
        assert launches(kernels) == {"transform_fast_kernel": 1}, kernels  # ... by the copy: the queued four-node chain


@pytest.mark.gpu
def test_a_two_column_node_reads_the_frame():
    def program(w):
        w.node(abi.Plus, "ts", OFF, "A")
        w.node(abi.Floor, "A", 3600, "B")
        w.two_columns(abi.Minus, "A", "B", "C")  # seconds into the local hour: no chain — both frames are written first
        return w.read_frame("C"), w.read_frame("A"), w.read_frame("B")
    got, want, kernels = both(program)
    assert got == want
    if _on():
        assert launches(kernels) == {"transform_fast_kernel": 2, "transform32_kernel": 1}, kernels


@pytest.mark.gpu
def test_the_source_column_is_rewritten_between_definition_and_use():
    def program(w):
        w.node(abi.Plus, "ts", OFF, "A")
        w.rewrite_column(77)  # the definition is written first: the frame holds the OLD timestamps' local time
        w.root(abi.Floor, "A", 3600)
        return w.read_dim(), w.read_frame("A")
    got, want, kernels = both(program)
    assert got == want
    if _on():
        assert launches(kernels).get("transform_fast_kernel") == 1, kernels


@pytest.mark.gpu
def test_the_defining_stream_is_destroyed():
    hip = H.hip_backend()
    s = hip.call("CreateCudaStream", 0)
    w = World(hip, stream=s)
    hip.wait(s)
    hip.profiler_enable(True)
    try:
        w.node(abi.Plus, "ts", OFF, "A")
        hip.wait(s)
        hip.call("DestroyCudaStream", s, 0)
        hip.wait()
        kernels = hip.profiler_report()
    finally:
        hip.profiler_enable(False)
    if _on():
        assert not launches(kernels), kernels  # retired with its stream
    # the frame's next definition, on another stream, is its own
    w.stream = None
    hip.call("InitIndexVector", w.idx.ptr, 0, w.n, None, 0)
    w.node(abi.Plus, "ts", 19800, "A")
    got = w.read_frame("A")
    w.free()
    wo = World(H.oracle_backend())
    wo.node(abi.Plus, "ts", 19800, "A")
    assert got == wo.read_frame("A")
    wo.free()


_GLOBAL_SCRIPT = r"""
import os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import harness as H
import test_chain_deferral as T
from aresdb_amd import abi
def program(w):
    w.node(abi.Plus, "ts", T.OFF, "A")
    w.node(abi.Mod, "A", 86400, "B")
    w.root(abi.Floor, "B", 3600)
    w.measure()
    w.be.wait(w.stream)
    w.replace_frame("A"); w.replace_frame("B")
    return w.hash_reduce()
got, want, kernels = T.both(program)
assert got == want and len(got) >= 25, (len(got), len(want))
print("KERNELS", sorted(T.launches(kernels).items()))
"""


@pytest.mark.gpu
def test_a_fallback_launches_the_queued_chain():
    """ARES_HASH_REDUCE=global: HashReduce declines the queue, which is launched — the chain job beside the measure's, in one
    transform_multi_kernel — and the frames, freed unread, were never written"""
    r = subprocess.run([sys.executable, "-c", _GLOBAL_SCRIPT], cwd=H.ROOT, env={**os.environ, "ARES_HASH_REDUCE": "global"},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    if _on():
        assert "KERNELS [('transform_multi_kernel', 1)]" in r.stdout, r.stdout[-1000:]


# ---- a seeded random interleaving --------------------------------------------------------------------------------------------
PROGRAMS, ROWS = 160, 3000
_FUNCTORS = (abi.Plus, abi.Minus, abi.Multiply, abi.Divide, abi.Mod, abi.Floor)
_CONSTS = (OFF, 19800, 345600, 86400, 604800, 3600, 7, 1, -3600)  # (no zero: the reference's division by zero is undefined)


def run_programs(be, seed=5, programs=PROGRAMS):
    """`programs` short programs over one world each; a digest of every buffer read, in order"""
    out = []
    for p in range(programs):
        rng = np.random.default_rng(seed * 1000 + p)
        w = World(be, n=ROWS, seed=seed + p)
        defined = set()
        for _ in range(int(rng.integers(4, 13))):
            op = rng.choice(["filter", "define", "chain", "inplace", "root", "two", "readf", "readd", "free", "rewrite", "wait", "init"],
                            p=[.06, .2, .16, .08, .14, .05, .1, .07, .05, .04, .03, .02])
            k = str(rng.choice(list("ABC")))
            f, c = int(rng.choice(_FUNCTORS)), int(rng.choice(_CONSTS))
            if op == "filter":
                w.filter(abi.GreaterThanOrEqual, int(rng.choice([0, 3600, 5 * 86400])))
                out.append(("count", p, w.size))
                if w.size == 0:
                    break
            elif op == "define":
                w.node(f, "ts", c, k)
                defined.add(k)
            elif op in ("chain", "inplace") and defined:
                src = str(rng.choice(sorted(defined)))
                dst = src if op == "inplace" else k
                w.node(f, src, c, dst)
                defined.add(dst)
            elif op == "root" and defined:
                w.root(f, str(rng.choice(sorted(defined))), c)
            elif op == "two" and len(defined) >= 2:
                a, b = (str(x) for x in rng.choice(sorted(defined), 2, replace=False))
                w.two_columns(abi.Minus, a, b, k)
                defined.add(k)
            elif op == "readf" and k in defined:
                out.append(("frame", p, hashlib.sha1(w.read_frame(k)).hexdigest()))
            elif op == "readd":
                out.append(("dim", p, hashlib.sha1(w.read_dim()).hexdigest()))
            elif op == "free" and k in defined:
                w.replace_frame(k)
                defined.discard(k)
            elif op == "rewrite":
                w.rewrite_column(int(rng.integers(1, 1000)))
            elif op == "wait":
                be.wait(w.stream)
            elif op == "init":
                be.call("InitIndexVector", w.idx.ptr, 0, w.n, w.stream, 0)
                w.size = w.n
        for k in sorted(defined):
            out.append(("frame_end", p, hashlib.sha1(w.read_frame(k)).hexdigest()))
        out.append(("dim_end", p, hashlib.sha1(w.read_dim()).hexdigest()))
        w.free()
    return [list(x) for x in out]


_FUZZ_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import harness as H
import test_chain_deferral as T
print("DIGESTS " + json.dumps(T.run_programs(H.hip_backend())))
"""


@pytest.mark.gpu
def test_random_interleavings_read_what_the_eager_sequence_leaves():
    want = run_programs(H.oracle_backend())
    got = run_programs(H.hip_backend())
    assert len(want) > 2 * PROGRAMS
    assert got == want
    r = subprocess.run([sys.executable, "-c", _FUZZ_SCRIPT], cwd=H.ROOT, env={**os.environ, "ARES_DEFER": "0"}, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    eager = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("DIGESTS ")][0][len("DIGESTS "):])
    assert eager == got
