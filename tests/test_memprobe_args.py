"""The memory probe without a GPU: its ring (native/include/vgpu/memprobe.h) exactly, and what its
entry points refuse (native/include/vgpu/calib_args.h).

Every refusal is tested here and nowhere else: tests/test_gpu_memprobe.py makes no call whose
arguments are meant to be refused, so a broken check can never start a kernel on a GPU.

* The definitions: vgpu_ring_next and vgpu_ring_jump of libvgpu_kernels.so (host-only exports, no
  HIP call) against ring_reference, against walking the ring, and against Python integers.
* The C entry points through ctypes in one child process from which every GPU is hidden: a
  refused call returns -1 before any HIP call, one that passes the checks reaches the launch and
  returns -2 for want of a device. The child makes no call at all if it can see a device.
* The Python wrappers: ValueError before the library is touched (a stand-in for the library
  fails the test if a call reaches it).
* native/tests/memprobe_host.cpp, the header's functions at their bound values in a stand-alone
  program built with -fsanitize=address,undefined.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import run_child

from amdvgpu.ops import calib, mem_chase, mem_latency, mem_stream, ring_build, ring_jump, ring_reference
from amdvgpu.shim.native import LIB_DIR

SEEDS = [0, 0x5EED, 0xFFFFFFFF]
MAX_STEPS, MAX_PASSES, MAX_WAVES = 1 << 18, 1 << 20, 16384

# Pointer arguments are named as in tests/test_calib_args.py: "A" and "B" are two 128-byte aligned
# host buffers of the child (never dereferenced: no call here reaches a GPU), "A+4" is four bytes
# into A, "NULL" is null.


def _chase(L=6, nblocks=1, lanes=1, steps=1, ring="A", out="B"):
    return ("vgpu_mem_chase", [ring, L, 7, nblocks, lanes, steps, 0, 0, out, "NULL"])


def _stream(buf="A", n_vec=8, mode=0, waves=4, duration_us=0, max_passes=1, out="B"):
    return ("vgpu_mem_stream", [buf, n_vec, mode, waves, duration_us, max_passes, 0, 7, out, "NULL"])


REFUSED = {}
for _L in (0, 26, -1):
    REFUSED[f"build-L={_L}"] = ("vgpu_ring_build", ["A", _L, 7, "NULL"])
    REFUSED[f"chase-L={_L}"] = _chase(L=_L)
REFUSED["build-ring=NULL"] = ("vgpu_ring_build", ["NULL", 1, 7, "NULL"])
for _off in (4, 16, 64):
    REFUSED[f"build-ring=A+{_off}"] = ("vgpu_ring_build", [f"A+{_off}", 1, 7, "NULL"])
REFUSED["chase-ring=NULL"] = _chase(ring="NULL")
REFUSED["chase-out=NULL"] = _chase(out="NULL")
for _nb in (0, 4097):
    REFUSED[f"chase-nblocks={_nb}"] = _chase(nblocks=_nb)
for _lanes in (0, 65):
    REFUSED[f"chase-lanes={_lanes}"] = _chase(lanes=_lanes)
for _steps in (0, MAX_STEPS + 1):
    REFUSED[f"chase-steps={_steps}"] = _chase(steps=_steps)
for _waves in (0, 3, 16388):
    REFUSED[f"stream-waves={_waves}"] = _stream(waves=_waves, n_vec=1 << 20)
REFUSED["stream-n_vec<waves"] = _stream(n_vec=7, waves=8)
REFUSED["stream-mode=2"] = _stream(mode=2)
for _us in (-1, 1000001):
    REFUSED[f"stream-duration_us={_us}"] = _stream(duration_us=_us)
for _p in (0, MAX_PASSES + 1):
    REFUSED[f"stream-max_passes={_p}"] = _stream(max_passes=_p)
REFUSED["stream-buf=NULL"] = _stream(buf="NULL")
REFUSED["stream-out=NULL"] = _stream(out="NULL")
for _off in (4, 8):
    REFUSED[f"stream-buf=A+{_off}"] = _stream(buf=f"A+{_off}")
    REFUSED[f"stream-out=B+{_off}"] = _stream(out=f"B+{_off}")

# The inner side of every bound: past the checks, and -2 because the child sees no device.
LAUNCHED = {
    "build-L=1": ("vgpu_ring_build", ["A", 1, 7, "NULL"]),
    "build-L=25": ("vgpu_ring_build", ["A", 25, 7, "NULL"]),
    "chase-min": _chase(L=1),
    "chase-max": _chase(L=25, nblocks=4096, lanes=64, steps=MAX_STEPS),
    "chase-unaligned": _chase(ring="A+4", out="B+4"),
    "stream-min": _stream(n_vec=4, waves=4),
    "stream-max": _stream(n_vec=MAX_WAVES, mode=1, waves=MAX_WAVES, duration_us=1000000, max_passes=MAX_PASSES),
    "stream-16-aligned": _stream(buf="A+16", out="B+16"),
}

JUMPS = [(L, seed) for L in (1, 6, 13) for seed in SEEDS]
BIG_K = [1 << 32, ((1 << 40) * 1000) % (1 << 64), (1 << 64) - 1]

CHILD = """
import ctypes
from amdvgpu.ops.calib import _k
L = _k()
n = ctypes.c_int(-1)
rc = L.hipGetDeviceCount(ctypes.byref(n))       # resolved through the library's dependencies
devices = n.value if rc == 0 else 0
bufs = {k: ctypes.create_string_buffer(256 + 128) for k in "AB"}

def ptr(name):
    if name == "NULL":
        return None
    base, _, off = name.partition("+")
    return ((ctypes.addressof(bufs[base]) + 127) & ~127) + int(off or 0)

def call(fn, args):
    return getattr(L, fn)(*[ptr(a) if isinstance(a, str) else a for a in args])

res = {}
if devices == 0:
    res = {group: {k: call(*v) for k, v in cases.items()} for group, cases in %r.items()}
emit(devices=devices, **res)
"""


@pytest.fixture(scope="module")
def rcs():
    cases = {"refused": {k: list(v) for k, v in REFUSED.items()}, "launched": {k: list(v) for k, v in LAUNCHED.items()}}
    res, _ = run_child(CHILD % (cases,), None, timeout=120,
                       extra_env={"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    assert res[0]["devices"] == 0, "a GPU is visible to the child: it made no call"
    return res[0]


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_c_entry_refuses(rcs, case):
    assert rcs["refused"][case] == -1, (case, REFUSED[case])


@pytest.mark.parametrize("case", sorted(LAUNCHED))
def test_c_entry_accepts_up_to_the_bounds(rcs, case):
    """-2: past the checks, and the launch failed because the child sees no device."""
    assert rcs["launched"][case] == -2, (case, LAUNCHED[case])


# ---- the definitions, exact (host-only exports: no HIP call, so no child is needed)

@pytest.fixture(scope="module")
def lib():
    return calib._k()


def _walk(ref, start, k):
    at = start
    for _ in range(k):
        at = int(ref[at])
    return at


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("L", [1, 2, 6, 13])
def test_c_ring_next_equals_the_reference(lib, L, seed):
    ref = ring_reference(L, seed)
    assert ref.dtype == np.uint32 and ref.shape == (1 << L,)
    got = np.array([lib.vgpu_ring_next(i, L, seed) for i in range(1 << L)], dtype=np.uint32)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("L", [1, 2, 3, 10, 16])
def test_ring_is_one_cycle(L, seed):
    ref = ring_reference(L, seed).tolist()
    n, at, seen = 1 << L, 0, set()
    for _ in range(n):
        assert at not in seen, "the walk came back early"
        seen.add(at)
        at = ref[at]
    assert at == 0 and len(seen) == n


@pytest.mark.parametrize("L, seed", JUMPS)
def test_ring_jump_equals_walking(lib, L, seed):
    n, ref = 1 << L, ring_reference(L, seed)
    for start in (0, n - 1):
        for k in (0, 1, 2, n - 1, n, n + 1, 1000):
            want = _walk(ref, start, k)
            assert lib.vgpu_ring_jump(start, k, L, seed) == want, (start, k)
            assert ring_jump(start, k, L, seed) == want, (start, k)


@pytest.mark.parametrize("L, seed", JUMPS)
def test_ring_jump_of_a_64_bit_count(lib, L, seed):
    """Against Python integers: k steps are k mod n steps, whatever k's size."""
    n, ref = 1 << L, ring_reference(L, seed)
    for k in BIG_K:
        want = _walk(ref, 3 % n, k % n)
        assert lib.vgpu_ring_jump(3 % n, k, L, seed) == want, k
        assert ring_jump(3 % n, k, L, seed) == want, k
    ks = np.array(BIG_K + [0, 1, n + 1], dtype=np.uint64)
    assert ring_jump(3 % n, ks, L, seed).tolist() == [ring_jump(3 % n, int(k), L, seed) for k in ks]


def test_ring_depends_on_the_seed():
    assert not np.array_equal(ring_reference(13, 1), ring_reference(13, 2))


def test_ring_exports_refuse_l_outside_the_range(lib):
    for L in (0, 26, -1):
        assert lib.vgpu_ring_next(0, L, 7) == 0xFFFFFFFF and lib.vgpu_ring_jump(0, 1, L, 7) == 0xFFFFFFFF
        with pytest.raises(ValueError, match="L "):
            ring_reference(L, 7)
        with pytest.raises(ValueError, match="L "):
            ring_jump(0, 1, L, 7)


@pytest.mark.parametrize("L, nblocks, warm", [(7, 256, True), (13, 64, True), (19, 64, True), (19, 256, True),
                                               (19, 50, True), (21, 64, True), (24, 64, False), (24, 256, False),
                                               (24, 50, False), (25, 256, False)])
def test_default_steps_cover_the_ring(L, nblocks, warm):
    """One lane per wave: block b is chain 64 b. A warm launch's chains cover the whole ring; a cold
    launch's chains overlap neither each other nor those of another chain_base."""
    n, steps = 1 << L, calib.chase_steps(1 << L, nblocks, warm)
    assert 1024 <= steps <= MAX_STEPS
    visits = np.zeros(n, dtype=np.int32)
    for base in ((0,) if warm else (0, 1, 63)):
        for b in range(nblocks):
            np.add.at(visits, ((base + 64 * b) * steps + np.arange(steps)) % n, 1)
    if warm:
        assert visits.min() >= 1
    else:
        assert visits.max() == 1 and visits.sum() == 3 * nblocks * steps


# ---- the Python wrappers

class _Untouchable:
    """In place of the loaded library: a wrapper that gets as far as calling it has not refused."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it has to refuse")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(calib, "_lib", _Untouchable())


class _OnDevice:
    """A contiguous tensor as the wrappers see one, claiming to live on a CUDA device."""
    is_cuda = True
    dtype = torch.int32
    device = torch.device("cuda:0")

    def __init__(self, addr, nbytes):
        self.addr, self.nbytes = addr, nbytes

    def numel(self): return self.nbytes // 4
    def element_size(self): return 4
    def is_contiguous(self): return True
    def data_ptr(self): return self.addr


RING = _OnDevice(0x10000, 128 << 6)
BUF = _OnDevice(0x20000, 16 * 64)


@pytest.mark.parametrize("L", [0, 26, -1])
def test_wrappers_refuse_l(no_library, L):
    with pytest.raises(ValueError, match="L "):
        ring_build(RING, L, 7)
    with pytest.raises(ValueError, match="L "):
        mem_chase(RING, L, 7, 1, 1, 1)


@pytest.mark.parametrize("nbytes", [0, 255, 128 << 26, 3 << 20])
def test_mem_latency_refuses_sizes(no_library, nbytes):
    with pytest.raises(ValueError, match="power of two"):
        mem_latency(nbytes)


def test_ring_build_refuses_tensors(no_library):
    with pytest.raises(ValueError, match="aligned"):
        ring_build(_OnDevice(0x10010, 128 << 6), 6, 7)
    with pytest.raises(ValueError, match="at least"):
        ring_build(_OnDevice(0x10000, (128 << 6) - 4), 6, 7)
    with pytest.raises(ValueError, match="CUDA"):
        ring_build(_cpu_aligned(128 << 6, 128), 6, 7)
    with pytest.raises(ValueError, match="contiguous"):
        ring_build(_cpu_aligned(2 * (128 << 6), 128)[::2], 6, 7)


def _cpu_aligned(nbytes, align):
    """A CPU int32 tensor of nbytes whose data_ptr() is `align`-byte aligned."""
    t = torch.zeros(nbytes + align, dtype=torch.uint8)
    off = -t.data_ptr() % align
    return t[off:off + nbytes].view(torch.int32)


@pytest.mark.parametrize("kw, why", [
    (dict(nblocks=0), "nblocks"), (dict(nblocks=4097), "nblocks"), (dict(lanes=0), "lanes"), (dict(lanes=65), "lanes"),
    (dict(steps=0), "steps"), (dict(steps=MAX_STEPS + 1), "steps"), (dict(first=64), "first"), (dict(first=-1), "first"),
    (dict(chain_base=-1), "chain_base"), (dict(chain_base=1 << 64), "chain_base"),
])
def test_mem_chase_refuses(no_library, kw, why):
    args = dict(nblocks=1, lanes=1, steps=1)
    args.update(kw)
    with pytest.raises(ValueError, match=why):
        mem_chase(RING, 6, 7, **args)


def test_mem_chase_refuses_tensors(no_library):
    with pytest.raises(ValueError, match="at least"):
        mem_chase(RING, 7, 7, 1, 1, 1)                       # a ring of 2**7 slots does not fit
    with pytest.raises(ValueError, match="CUDA"):
        mem_chase(_cpu_aligned(128 << 6, 128), 6, 7, 1, 1, 1)
    with pytest.raises(ValueError, match="out is"):
        mem_chase(RING, 6, 7, 1, 1, 1, out=_OnDevice(0x30000, 4 * 511))


@pytest.mark.parametrize("kw, why", [
    (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(mode="both"), "mode"),
    (dict(waves=0), "waves"), (dict(waves=3), "waves"), (dict(waves=16388), "waves"), (dict(waves=68), "n_vec"),
    (dict(duration_us=-1), "duration_us"), (dict(duration_us=1000001), "duration_us"),
    (dict(max_passes=0), "max_passes"), (dict(max_passes=MAX_PASSES + 1), "max_passes"),
    (dict(seed=1 << 32), "seed"), (dict(base=-1), "seed"),
])
def test_mem_stream_refuses(no_library, kw, why):
    args = dict(mode=0, waves=4, duration_us=0, max_passes=1, seed=7)
    args.update(kw)
    with pytest.raises(ValueError, match=why):
        mem_stream(BUF, **args)


def test_mem_stream_refuses_tensors(no_library):
    with pytest.raises(ValueError, match="multiple of 16"):
        mem_stream(_OnDevice(0x20000, 16 * 64 + 8), 0, 4, 0, 1, 7)
    with pytest.raises(ValueError, match="aligned"):
        mem_stream(_OnDevice(0x20008, 16 * 64), 0, 4, 0, 1, 7)
    with pytest.raises(ValueError, match="CUDA"):
        mem_stream(_cpu_aligned(16 * 64, 16), 0, 4, 0, 1, 7)
    with pytest.raises(ValueError, match="contiguous"):
        mem_stream(_cpu_aligned(2 * 16 * 64, 16)[::2], 0, 4, 0, 1, 7)
    with pytest.raises(ValueError, match="out is"):
        mem_stream(BUF, 0, 4, 0, 1, 7, out=_OnDevice(0x30000, 4 * 31))
    with pytest.raises(ValueError, match="aligned"):
        mem_stream(BUF, 0, 4, 0, 1, 7, out=_OnDevice(0x30008, 4 * 32))


@pytest.mark.parametrize("argv", [["--sizes", "3m"], ["--sizes", "128"], ["--sizes", "8g"], ["--stream-ms", "1001"]])
def test_cli_refuses_before_touching_a_gpu(no_library, argv):
    from amdvgpu.cli import main
    with pytest.raises(SystemExit) as e:
        main(["memprobe", *argv])
    assert e.value.code == 2


# ---- the host program under AddressSanitizer and UBSan

def test_host_program_under_sanitizers():
    """native/tests/memprobe_host.cpp, built by the Makefile with -fsanitize=address,undefined and
    the runtimes linked in statically: nothing is preloaded."""
    exe = os.path.join(LIB_DIR, "memprobe_host")
    assert os.path.exists(exe), "the native build did not produce memprobe_host"
    with open(exe, "rb") as f:
        assert b"__asan_init" in f.read(), "memprobe_host was built without AddressSanitizer"
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "memprobe_host ok" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
