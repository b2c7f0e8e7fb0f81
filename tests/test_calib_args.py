"""What the calibration entry points refuse (native/include/vgpu/calib_args.h), without a GPU.

Every refusal is tested here and nowhere else: tests/test_gpu_calib.py makes no call whose
arguments are meant to be refused, so a broken check can never start a kernel on a GPU.

* The C entry points of libvgpu_kernels.so, through ctypes in one child process from which
  every GPU is hidden: a refused call returns -1 before any HIP call, one that slips past the
  checks reaches the launch and returns -2 for want of a device. The child makes no call at
  all if it can see a device.
* The Python wrappers: ValueError before the library is touched (a stand-in for the library
  fails the test if a call reaches it).
* scratch_reference, the numpy simulation of scratch_kernel, against a second formulation.
"""
import numpy as np
import pytest
import torch

from conftest import run_child

from amdvgpu.ops import calib, cu_census, scratch_hog, scratch_reference, spin, spin_lds, stream_copy

INT_MIN, INT_MAX = -2**31, 2**31 - 1
MAX_BLOCKS, MAX_SPIN_US, MAX_LDS = 1 << 20, 1000000, 163840

# Pointer arguments are named: "A" and "B" are two 16-byte aligned host buffers of the child
# (never dereferenced: no call here reaches a GPU), "A+4" is four bytes into A, "NULL" is null.
SPINNERS = {
    "census": ("vgpu_cu_census", lambda nb, us: ["A", nb, us, "NULL"]),
    "spin": ("vgpu_spin", lambda nb, us: [nb, us, "NULL", "NULL"]),
    "spin_lds": ("vgpu_spin_lds", lambda nb, us: [nb, us, 1024, "NULL"]),
}
REFUSED = {}
for _name, (_fn, _args) in SPINNERS.items():
    for _nb in (0, -1, INT_MIN, MAX_BLOCKS + 1, INT_MAX):
        REFUSED[f"{_name}-nblocks={_nb}"] = (_fn, _args(_nb, 10))
    for _us in (-1, INT_MIN, MAX_SPIN_US + 1, INT_MAX):
        REFUSED[f"{_name}-spin_us={_us}"] = (_fn, _args(1, _us))
REFUSED["census-out=NULL"] = ("vgpu_cu_census", ["NULL", 1, 10, "NULL"])
for _lds in (0, -1, INT_MIN, MAX_LDS + 1, INT_MAX):
    REFUSED[f"spin_lds-lds_bytes={_lds}"] = ("vgpu_spin_lds", [1, 10, _lds, "NULL"])
REFUSED["scratch-out=NULL"] = ("vgpu_scratch_hog", ["NULL", 1, 3, "NULL"])
for _nb in (0, -1, INT_MIN, MAX_BLOCKS + 1, INT_MAX):
    REFUSED[f"scratch-nblocks={_nb}"] = ("vgpu_scratch_hog", ["A", _nb, 3, "NULL"])
for _stride in (0, 2, 4096, -1, -3, INT_MIN, INT_MIN + 1, INT_MAX - 1):
    REFUSED[f"scratch-stride={_stride}"] = ("vgpu_scratch_hog", ["A", 1, _stride, "NULL"])
REFUSED["copy-dst=NULL"] = ("vgpu_stream_copy", ["NULL", "B", 16, "NULL"])
REFUSED["copy-src=NULL"] = ("vgpu_stream_copy", ["A", "NULL", 16, "NULL"])
REFUSED["copy-both=NULL-bytes=0"] = ("vgpu_stream_copy", ["NULL", "NULL", 0, "NULL"])
for _n in (1, 8, 15, 17, 24, 2**40 + 8):
    REFUSED[f"copy-bytes={_n}"] = ("vgpu_stream_copy", ["A", "B", _n, "NULL"])
for _off in (1, 4, 8, 15):
    REFUSED[f"copy-dst=A+{_off}"] = ("vgpu_stream_copy", [f"A+{_off}", "B", 16, "NULL"])
    REFUSED[f"copy-src=B+{_off}"] = ("vgpu_stream_copy", ["A", f"B+{_off}", 16, "NULL"])
REFUSED["copy-dst=A+8-bytes=0"] = ("vgpu_stream_copy", ["A+8", "B", 0, "NULL"])
REFUSED["copy-src=B+8-bytes=0"] = ("vgpu_stream_copy", ["A", "B+8", 0, "NULL"])

# Accepted arguments at the bounds' inner side: with no device the launch fails, -2. They show
# that -1 above is the check's answer and not the library's answer to everything.
LAUNCHED = {
    "census": ("vgpu_cu_census", ["A", 1, 0, "NULL"]),
    "census-max": ("vgpu_cu_census", ["A", MAX_BLOCKS, MAX_SPIN_US, "NULL"]),
    "spin": ("vgpu_spin", [1, 0, "NULL", "NULL"]),
    "spin-max": ("vgpu_spin", [MAX_BLOCKS, MAX_SPIN_US, "NULL", "NULL"]),
    "spin_lds-min": ("vgpu_spin_lds", [1, 0, 1, "NULL"]),
    "spin_lds-max": ("vgpu_spin_lds", [MAX_BLOCKS, MAX_SPIN_US, MAX_LDS, "NULL"]),
    "scratch-stride=1": ("vgpu_scratch_hog", ["A", 1, 1, "NULL"]),
    "scratch-max": ("vgpu_scratch_hog", ["A", MAX_BLOCKS, INT_MAX, "NULL"]),
    "copy": ("vgpu_stream_copy", ["A", "B", 16, "NULL"]),
}

CHILD = """
import ctypes
from amdvgpu.ops.calib import _k
L = _k()
n = ctypes.c_int(-1)
rc = L.hipGetDeviceCount(ctypes.byref(n))       # resolved through the library's dependencies
devices = n.value if rc == 0 else 0
bufs = {k: ctypes.create_string_buffer(256 + 16) for k in "AB"}

def ptr(name):
    if name == "NULL":
        return None
    base, _, off = name.partition("+")
    return ((ctypes.addressof(bufs[base]) + 15) & ~15) + int(off or 0)

def call(fn, args):
    return getattr(L, fn)(*[ptr(a) if isinstance(a, str) else a for a in args])

res = {}
if devices == 0:
    res = {group: {k: call(*v) for k, v in cases.items()} for group, cases in %r.items()}
    res["nothing"] = call("vgpu_stream_copy", ["A", "B", 0, "NULL"])
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


def test_c_copy_of_zero_bytes_launches_nothing(rcs):
    assert rcs["nothing"] == 0


class _Untouchable:
    """In place of the loaded library: a wrapper that gets as far as calling it has not refused."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name}) with arguments it has to refuse")


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(calib, "_lib", _Untouchable())


@pytest.mark.parametrize("nblocks", [0, -1, MAX_BLOCKS + 1, INT_MIN])
@pytest.mark.parametrize("fn", [lambda nb: cu_census(nb, 10), lambda nb: spin(nb, 10), lambda nb: spin_lds(nb, 10, 1024),
                                lambda nb: scratch_hog(nb)], ids=["cu_census", "spin", "spin_lds", "scratch_hog"])
def test_wrapper_refuses_nblocks(no_library, fn, nblocks):
    with pytest.raises(ValueError, match="nblocks"):
        fn(nblocks)


@pytest.mark.parametrize("spin_us", [-1, INT_MIN, MAX_SPIN_US + 1])
@pytest.mark.parametrize("fn", [lambda us: cu_census(1, us), lambda us: spin(1, us), lambda us: spin_lds(1, us, 1024)],
                         ids=["cu_census", "spin", "spin_lds"])
def test_wrapper_refuses_spin_us(no_library, fn, spin_us):
    with pytest.raises(ValueError, match="spin_us"):
        fn(spin_us)


@pytest.mark.parametrize("lds_bytes", [0, -1, MAX_LDS + 1])
def test_spin_lds_refuses_lds_bytes(no_library, lds_bytes):
    with pytest.raises(ValueError, match="lds_bytes"):
        spin_lds(1, 10, lds_bytes)


@pytest.mark.parametrize("stride", [0, 2, 4096, -1, -3, 2**31, 2**31 + 1, 2**32 + 1])
def test_scratch_refuses_stride(no_library, stride):
    with pytest.raises(ValueError, match="stride"):
        scratch_hog(1, stride)
    with pytest.raises(ValueError, match="stride"):
        scratch_reference(stride)


@pytest.mark.parametrize("counter, why", [
    (torch.zeros(1, dtype=torch.int32), "int64"),
    (torch.zeros(1, dtype=torch.float64), "int64"),
    ([0], "int64"),
    (torch.zeros(0, dtype=torch.int64), "at least one element"),
    (torch.zeros(1, dtype=torch.int64), "CUDA"),
], ids=["int32", "float64", "list", "empty", "cpu"])
def test_spin_refuses_counter(no_library, counter, why):
    with pytest.raises(ValueError, match=why):
        spin(1, 10, counter=counter)


def _aligned(nbytes):
    """A CPU uint8 tensor of nbytes whose data_ptr() is 16-byte aligned."""
    t = torch.zeros(nbytes + 16, dtype=torch.uint8)
    off = -t.data_ptr() % 16
    return t[off:off + nbytes]


class _OnDevice:
    """A contiguous, aligned tensor as stream_copy sees one, claiming to live on a CUDA device:
    two CUDA devices do not exist where this test runs."""
    is_cuda = True

    def __init__(self, addr, device):
        self.addr, self.device = addr, torch.device(device)

    def numel(self): return 64
    def element_size(self): return 1
    def is_contiguous(self): return True
    def data_ptr(self): return self.addr


def test_stream_copy_refuses_cpu_tensors(no_library):
    a, b = _aligned(64), _aligned(64)
    with pytest.raises(ValueError, match="CUDA"):
        stream_copy(a, b)
    with pytest.raises(ValueError, match="CUDA"):
        stream_copy(_OnDevice(0x1000, "cuda:0"), b)
    with pytest.raises(ValueError, match="CUDA"):
        stream_copy(a, _OnDevice(0x1000, "cuda:0"))
    with pytest.raises(ValueError, match="CUDA"):
        stream_copy(a, b, 0)


def test_stream_copy_refuses_different_devices(no_library):
    with pytest.raises(ValueError, match="different devices"):
        stream_copy(_OnDevice(0x1000, "cuda:0"), _OnDevice(0x2000, "cuda:1"))


def test_stream_copy_refuses_strided_views(no_library):
    a, b = _aligned(128), _aligned(128)
    with pytest.raises(ValueError, match="contiguous"):
        stream_copy(a[::2], b[:64])
    with pytest.raises(ValueError, match="contiguous"):
        stream_copy(a[:64], b[::2])
    with pytest.raises(ValueError, match="contiguous"):
        stream_copy(a.view(8, 16).t(), b)


@pytest.mark.parametrize("off", [1, 4, 8, 15])
def test_stream_copy_refuses_misaligned_tensors(no_library, off):
    a, b = _aligned(64), _aligned(64)
    with pytest.raises(ValueError, match="aligned"):
        stream_copy(a[off:off + 16], b[:16])
    with pytest.raises(ValueError, match="aligned"):
        stream_copy(a[:16], b[off:off + 16])


def test_stream_copy_refuses_overlapping_ranges(no_library):
    a = _aligned(128)
    with pytest.raises(ValueError, match="overlapping"):
        stream_copy(a, a)
    with pytest.raises(ValueError, match="overlapping"):
        stream_copy(a[16:80], a[:64])
    with pytest.raises(ValueError, match="overlapping"):
        stream_copy(a[:64], a[48:112])
    with pytest.raises(ValueError, match="CUDA"):          # adjacent ranges do not overlap
        stream_copy(a[:64], a[64:])
    with pytest.raises(ValueError, match="CUDA"):          # nor does the part that is copied
        stream_copy(a[:64], a[32:96], 32)


def test_stream_copy_refuses_sizes(no_library):
    a, b = _aligned(64), _aligned(64)
    with pytest.raises(ValueError, match="negative"):
        stream_copy(a, b, -16)
    with pytest.raises(ValueError, match="negative"):
        stream_copy(a, b, -1)
    with pytest.raises(ValueError, match="multiple of 16"):
        stream_copy(a, b, 24)
    with pytest.raises(ValueError, match="multiple of 16"):
        stream_copy(a[:24], b[:24])
    with pytest.raises(ValueError, match="larger"):
        stream_copy(a[:32], b)
    with pytest.raises(ValueError, match="larger"):
        stream_copy(a, b, 80)


def _scratch_second_formulation(stride):
    """Every read index j = i * stride mod 4096 was written once, by i' = (j - lane) / stride
    mod 4096, and holds i' ^ lane: the checksums without simulating the array."""
    inv = pow(stride, -1, 4096)
    lane = np.arange(64, dtype=np.int64).reshape(-1, 1)
    j = (np.arange(0, 4096, 7, dtype=np.int64) * (stride % 4096)) % 4096
    writer = ((j - lane) % 4096) * inv % 4096
    return ((writer ^ lane).sum(axis=1) & 0xFFFFFFFF).astype(np.uint32)


STRIDES = [1, 3, 4095, 506952113, 0x7FFFFFFF]


@pytest.mark.parametrize("stride", STRIDES)
def test_scratch_reference_agrees_with_a_second_formulation(stride):
    got = scratch_reference(stride)
    assert got.dtype == np.uint32 and got.shape == (64,)
    assert np.array_equal(got, _scratch_second_formulation(stride))
    assert len(set(got.tolist())) > 1, "every lane has the same checksum: a lane mix-up would not show"


def test_scratch_reference_depends_on_the_stride():
    assert not np.array_equal(scratch_reference(1), scratch_reference(3))
    assert calib.SCRATCH_STRIDE == 506952113
    assert np.array_equal(scratch_reference(), scratch_reference(506952113))
    assert len(set(scratch_reference().tolist())) == 64
