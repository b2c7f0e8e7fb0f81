"""gfx950 calibration kernels (native/src/kernels/vgpu_kernels.hip) driven from PyTorch.

These are the measurement instruments of the data plane:

* :func:`cu_census` launches long-spinning single-wave workgroups that each record the
  (XCC, SE, SH, CU) they ran on, read from HW_REG_XCC_ID / HW_REG_HW_ID. The number of
  distinct CUs observed is the spatial partition a queue is actually confined to.
* :func:`spin` fixed-duration workgroups for duty-cycle measurements of the temporal
  limiter; :func:`spin_lds` the same holding dynamic LDS.
* :func:`scratch_hog` lanes with a 16 KiB private array each; :func:`scratch_reference` is the
  same computation in numpy.
* :func:`stream_copy` 16 B/lane grid-stride copy: HBM bandwidth, or host-spill bandwidth
  when the source lives in spilled (host) memory.
* :func:`pattern_fill` / :func:`pattern_check` / :func:`pattern_poke` word-exact fill and
  verify at memory bandwidth (native/include/vgpu/pattern.h): integrity of buffers that the
  spill, promotion and demotion paths move. :func:`pattern_reference` is the same
  definition in numpy. ``vgpu-validate --conformance`` runs the same kernels in a pod.
* :func:`cu_selftest` four-wave workgroups whose every wave runs a known-answer test of the
  VALU, the LDS and the i8 and f16 matrix cores (native/include/vgpu/selftest.h) and records
  the CU and SIMD it ran on: which CU of the slice, and which unit of it, computes wrong.
  :func:`selftest_reference` is the same definition in numpy; ``vgpu-validate --conformance
  --compute`` runs the same kernel in a pod.
* :func:`ring_build` / :func:`mem_chase` / :func:`mem_latency` a pointer chase over a ring of
  128-byte slots (native/include/vgpu/memprobe.h): dependent vector loads stamped with the
  shader clock and the 100 MHz clock, the latency of whichever level of the memory hierarchy
  the ring fits. :func:`ring_reference` and :func:`ring_jump` are the ring in numpy, and every
  chain's end slot is checked against them.
* :func:`mem_stream` waves that read or write their own chunk of a buffer for a fixed time: a
  controlled memory load, checked against :func:`pattern_reference` word-exactly.

The wrappers refuse with ValueError what the C entry points refuse with -1
(native/include/vgpu/calib_args.h): no spin longer than a second or negative, no grid past
2**20 workgroups, no copy of strided, misaligned, overlapping or host tensors, no chase of more
than 2**18 steps or 4096 workgroups, no stream longer than a second.

The library is required: there is no PyTorch fallback, a missing build raises.
"""
import ctypes as C

from ..shim.native import KERNELS, lib_path

_lib = None


def _k():
    global _lib
    if _lib is None:
        L = C.CDLL(lib_path(KERNELS))
        L.vgpu_cu_census.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vgpu_cu_census.restype = C.c_int
        L.vgpu_spin.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.vgpu_spin.restype = C.c_int
        L.vgpu_spin_lds.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.vgpu_spin_lds.restype = C.c_int
        L.vgpu_stream_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vgpu_stream_copy.restype = C.c_int
        L.vgpu_scratch_hog.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.vgpu_scratch_hog.restype = C.c_int
        L.vgpu_pattern_fill.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_void_p]
        L.vgpu_pattern_fill.restype = C.c_int
        L.vgpu_pattern_check.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        L.vgpu_pattern_check.restype = C.c_int
        L.vgpu_pattern_poke.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.vgpu_pattern_poke.restype = C.c_int
        L.vgpu_cu_selftest.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                       C.c_void_p]
        L.vgpu_cu_selftest.restype = C.c_int
        L.vgpu_ring_next.argtypes = [C.c_uint32, C.c_int, C.c_uint32]
        L.vgpu_ring_next.restype = C.c_uint32
        L.vgpu_ring_jump.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.c_uint32]
        L.vgpu_ring_jump.restype = C.c_uint32
        L.vgpu_ring_build.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        L.vgpu_ring_build.restype = C.c_int
        L.vgpu_mem_chase.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64,
                                     C.c_void_p, C.c_void_p]
        L.vgpu_mem_chase.restype = C.c_int
        L.vgpu_mem_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint32,
                                      C.c_void_p, C.c_void_p]
        L.vgpu_mem_stream.restype = C.c_int
        _lib = L
    return _lib


def decode_location(code):
    """(xcc, se, sh, cu) from a census code."""
    code = int(code)
    return (code >> 12) & 0xF, (code >> 8) & 0xF, (code >> 4) & 0xF, code & 0xF


def _stream(torch, device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


MAX_BLOCKS = 1 << 20      # the bounds of native/include/vgpu/calib_args.h
MAX_SPIN_US = 1000000
MAX_LDS_BYTES = 160 * 1024
SCRATCH_WORDS = 4096      # 16 KiB of private memory per lane
SCRATCH_STRIDE = 2654435761 & 0x7FFFFFFF | 1


def _grid(nblocks, spin_us=0):
    """(nblocks, spin_us) as ints, refusing what the C entry points refuse: a spin outside
    0..1 s (a negative one would never return) or a grid outside 1..2**20 workgroups."""
    nblocks, spin_us = int(nblocks), int(spin_us)
    if not 1 <= nblocks <= MAX_BLOCKS:
        raise ValueError(f"nblocks {nblocks} outside 1..{MAX_BLOCKS}")
    if not 0 <= spin_us <= MAX_SPIN_US:
        raise ValueError(f"spin_us {spin_us} outside 0..{MAX_SPIN_US}")
    return nblocks, spin_us


def cu_census(nblocks=4096, spin_us=200, device=None):
    """Returns the set of distinct (xcc, se, sh, cu) tuples the workgroups ran on.
    ``nblocks`` in 1..2**20 and ``spin_us`` in 0..1000000, else ValueError."""
    import torch
    nblocks, spin_us = _grid(nblocks, spin_us)
    device = torch.device(device or "cuda")
    out = torch.zeros(nblocks, dtype=torch.int32, device=device)
    rc = _k().vgpu_cu_census(C.c_void_p(out.data_ptr()), nblocks, spin_us, _stream(torch, device))
    if rc != 0:
        raise RuntimeError(f"vgpu_cu_census launch failed ({rc})")
    torch.cuda.synchronize(device)
    return {decode_location(c) for c in out.cpu().tolist()}


def spin(nblocks, spin_us, device=None, counter=None):
    """Launches ``nblocks`` workgroups spinning ``spin_us`` each (asynchronous); every
    workgroup then adds 1 to element 0 of ``counter``, a CUDA int64 tensor, when one is given.
    ``nblocks`` in 1..2**20 and ``spin_us`` in 0..1000000, else ValueError."""
    import torch
    nblocks, spin_us = _grid(nblocks, spin_us)
    if counter is not None:
        if not isinstance(counter, torch.Tensor) or counter.dtype != torch.int64:
            raise ValueError("the counter must be an int64 tensor")
        if counter.numel() < 1:
            raise ValueError("the counter needs at least one element")
        if not counter.is_cuda:
            raise ValueError("the counter must be a CUDA tensor")
    device = torch.device(device or "cuda")
    ptr = C.c_void_p(counter.data_ptr()) if counter is not None else None
    rc = _k().vgpu_spin(nblocks, spin_us, ptr, _stream(torch, device))
    if rc != 0:
        raise RuntimeError(f"vgpu_spin launch failed ({rc})")


def spin_lds(nblocks, spin_us, lds_bytes, device=None):
    """Launches ``nblocks`` workgroups spinning ``spin_us`` each while holding
    ``lds_bytes`` of LDS (asynchronous): a grid dispatched over many rounds.
    ``nblocks`` in 1..2**20, ``spin_us`` in 0..1000000 and ``lds_bytes`` in 1..163840 (a CU's
    whole LDS), else ValueError."""
    import torch
    nblocks, spin_us = _grid(nblocks, spin_us)
    lds_bytes = int(lds_bytes)
    if not 1 <= lds_bytes <= MAX_LDS_BYTES:
        raise ValueError(f"lds_bytes {lds_bytes} outside 1..{MAX_LDS_BYTES}")
    device = torch.device(device or "cuda")
    rc = _k().vgpu_spin_lds(nblocks, spin_us, lds_bytes, _stream(torch, device))
    if rc != 0:
        raise RuntimeError(f"vgpu_spin_lds launch failed ({rc})")


def stream_copy(dst, src, nbytes=None):
    """Copies ``nbytes`` (default: all of src) from tensor src to tensor dst (asynchronous).

    Both are contiguous CUDA tensors of one device whose ``data_ptr()`` is 16-byte aligned and
    whose byte ranges do not overlap (the kernel's pointers are ``__restrict__``); ``nbytes`` is
    a multiple of 16 that fits both, and 0 copies nothing. Anything else is a ValueError."""
    import torch
    dst_bytes, src_bytes = dst.numel() * dst.element_size(), src.numel() * src.element_size()
    n = int(nbytes if nbytes is not None else src_bytes)
    if n < 0:
        raise ValueError("stream_copy of a negative size")
    if n > dst_bytes or n > src_bytes:
        raise ValueError("copy larger than a buffer")
    if n % 16:
        raise ValueError("stream_copy needs a multiple of 16 bytes")
    if not dst.is_contiguous() or not src.is_contiguous():
        raise ValueError("stream_copy needs contiguous tensors")
    if dst.data_ptr() % 16 or src.data_ptr() % 16:
        raise ValueError("stream_copy needs 16-byte aligned tensors")
    if dst.data_ptr() < src.data_ptr() + n and src.data_ptr() < dst.data_ptr() + n:
        raise ValueError("stream_copy of overlapping byte ranges")
    if not dst.is_cuda or not src.is_cuda:
        raise ValueError("stream_copy needs CUDA tensors")
    if dst.device != src.device:
        raise ValueError("stream_copy between tensors on different devices")
    if n == 0:
        return
    rc = _k().vgpu_stream_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, _stream(torch, dst.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_stream_copy launch failed ({rc})")


def scratch_reference(stride=SCRATCH_STRIDE):
    """The 64 checksums one workgroup of :func:`scratch_hog` writes, as uint32, simulated
    literally from scratch_kernel in numpy: each lane fills its 4096-word private array with
    ``buf[(i * stride + lane) % 4096] = i ^ lane`` for i in 0..4095 and then sums
    ``buf[(i * stride) % 4096]`` over i = 0, 7, 14, ..., all in 32-bit arithmetic."""
    import numpy as np
    stride = int(stride)
    if not 1 <= stride <= 0x7FFFFFFF or not stride & 1:
        raise ValueError("stride is odd and in 1..2**31-1")
    m32 = np.uint64(0xFFFFFFFF)
    words = np.uint64(SCRATCH_WORDS)
    lane = np.arange(64, dtype=np.uint64)
    rows = np.arange(64)
    buf = np.zeros((64, SCRATCH_WORDS), dtype=np.uint64)
    written = np.zeros((64, SCRATCH_WORDS), dtype=bool)
    for i in range(SCRATCH_WORDS):  # in the kernel's order: a later write to a word wins
        at = ((((np.uint64(i) * np.uint64(stride)) & m32) + lane) & m32) % words
        buf[rows, at] = np.uint64(i) ^ lane
        written[rows, at] = True
    acc = np.zeros(64, dtype=np.uint64)
    for i in range(0, SCRATCH_WORDS, 7):
        at = int(((np.uint64(i) * np.uint64(stride)) & m32) % words)
        assert written[:, at].all(), "the kernel would read a word it never wrote"
        acc = (acc + buf[:, at]) & m32
    return acc.astype(np.uint32)


def scratch_hog(nblocks=4096, stride=SCRATCH_STRIDE, device=None):
    """Runs a kernel whose lanes each hold a 16 KiB private (scratch) array; returns the
    per-lane checksums, 64 int32 per workgroup whose bits are :func:`scratch_reference`. ROCr
    backs the private segment with a scratch allocation that never passes the allocation hooks
    (the shim accounts it from KFD's VRAM counter). ``nblocks`` in 1..2**20 and ``stride`` odd
    and in 1..2**31-1, else ValueError."""
    import torch
    nblocks, _ = _grid(nblocks)
    stride = int(stride)
    if not 1 <= stride <= 0x7FFFFFFF or not stride & 1:
        raise ValueError("stride is odd and in 1..2**31-1")
    device = torch.device(device or "cuda")
    out = torch.empty(nblocks * 64, dtype=torch.int32, device=device)
    rc = _k().vgpu_scratch_hog(C.c_void_p(out.data_ptr()), nblocks, stride, _stream(torch, device))
    if rc != 0:
        raise RuntimeError(f"vgpu_scratch_hog launch failed ({rc})")
    return out


def pattern_reference(n_words, seed, base=0):
    """The test pattern in pure numpy: words ``base .. base + n_words`` under ``seed`` as
    uint32 (the definition of native/include/vgpu/pattern.h; ``base`` is a 64-bit word index)."""
    import numpy as np
    seed, base = int(seed), int(base)
    if not 0 <= seed < 1 << 32 or not 0 <= base or base + int(n_words) > 1 << 64:
        raise ValueError("seed is 32 bits, base + n_words at most 2**64")
    m32 = np.uint64(0xFFFFFFFF)
    idx = np.arange(int(n_words), dtype=np.uint64) + np.uint64(base)
    vec, lane = idx >> np.uint64(2), idx & np.uint64(3)
    # 32-bit arithmetic carried in uint64 and masked after every product and sum
    a = (((vec & m32) ^ np.uint64(seed)) * np.uint64(0x9E3779B1)) & m32
    a ^= a >> np.uint64(15)
    a = (a + (((vec >> np.uint64(32)) * np.uint64(0x85EBCA77)) & m32) + np.uint64(seed)) & m32
    a = (a * np.uint64(0xC2B2AE3D)) & m32
    a ^= a >> np.uint64(13)
    r = lane * np.uint64(8)
    rot = ((a << r) | (a >> ((np.uint64(32) - r) & np.uint64(31)))) & m32
    return ((rot + lane * np.uint64(0x9E3779B9)) & m32).astype(np.uint32)


def _pattern_bytes(t):
    n = t.numel() * t.element_size()
    if not t.is_contiguous():
        raise ValueError("the pattern kernels need a contiguous tensor")
    if n == 0 or n % 16:
        raise ValueError("the pattern kernels need a nonzero multiple of 16 bytes")
    if t.data_ptr() % 16:
        raise ValueError("the pattern kernels need a 16-byte aligned tensor")
    return n


def pattern_fill(t, seed, base=0):
    """Fills tensor ``t`` (a multiple of 16 bytes): its 32-bit word k becomes
    ``w(base + k, seed)`` (asynchronous)."""
    import torch
    n = _pattern_bytes(t)
    rc = _k().vgpu_pattern_fill(C.c_void_p(t.data_ptr()), n, int(base), int(seed), _stream(torch, t.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_pattern_fill launch failed ({rc})")


def pattern_check(t, seed, base=0):
    """Verifies tensor ``t`` against the pattern. Returns ``(mismatches, first_index)``:
    the number of 32-bit words that differ and the lowest such word index of ``t``
    (``None`` when there is none). Synchronises."""
    import torch
    n = _pattern_bytes(t)
    out = torch.tensor([0, -1], dtype=torch.int64, device=t.device)
    rc = _k().vgpu_pattern_check(C.c_void_p(t.data_ptr()), n, int(base), int(seed), C.c_void_p(out.data_ptr()),
                                 _stream(torch, t.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_pattern_check launch failed ({rc})")
    bad, first = out.cpu().tolist()
    return bad, (first if bad else None)


def pattern_poke(t, indices):
    """Flips one bit in each of the listed 32-bit words of ``t`` (asynchronous): proves that
    :func:`pattern_check` can fail."""
    import torch
    words = t.numel() * t.element_size() // 4
    indices = [int(i) for i in indices]
    if not indices:
        return
    if min(indices) < 0 or max(indices) >= words:
        raise ValueError("poke index outside the tensor")
    idx = torch.tensor(indices, dtype=torch.int64, device=t.device)
    rc = _k().vgpu_pattern_poke(C.c_void_p(t.data_ptr()), C.c_void_p(idx.data_ptr()), len(indices),
                                _stream(torch, t.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_pattern_poke launch failed ({rc})")
    torch.cuda.current_stream(t.device).synchronize()  # idx must outlive the kernel


SELFTEST_UNITS = ("valu", "lds", "mfma_i8", "mfma_f16")  # the order of a wave's four words
SELFTEST_MAX_ROUNDS = 1024
_M32 = 0xFFFFFFFF


def _selftest_hash(q, seed):
    """vgpu_pattern_hash for indices below 2**32, as uint64 carrying 32-bit values."""
    import numpy as np
    m32 = np.uint64(_M32)
    a = ((np.asarray(q, dtype=np.uint64) ^ np.uint64(seed)) * np.uint64(0x9E3779B1)) & m32
    a ^= a >> np.uint64(15)
    a = (a + np.uint64(seed)) & m32
    a = (a * np.uint64(0xC2B2AE3D)) & m32
    a ^= a >> np.uint64(13)
    return a


def _selftest_mix(x):
    import numpy as np
    m32 = np.uint64(_M32)
    x = np.asarray(x, dtype=np.uint64) & m32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x85EBCA77)) & m32
    return x ^ (x >> np.uint64(13))


def _selftest_fold(c):
    """fold() of a 32x32 integer matrix: position-dependent, 32-bit wrapping."""
    import numpy as np
    pos = (np.arange(1024, dtype=np.uint64).reshape(32, 32) * np.uint64(0x9E3779B9)) & np.uint64(_M32)
    c32 = (np.asarray(c, dtype=np.int64) & _M32).astype(np.uint64)
    return int(_selftest_mix(c32 + pos).sum()) & _M32


def selftest_accumulators(seed, rounds, inject=False):
    """The two 32x32 accumulators of the known-answer test as int64: (mfma_i8, mfma_f16).
    Asserts what the definition promises about them: the i8 accumulator stays below 2**29,
    every partial sum of the f16 one below 2**24, and a float32 accumulation of the f16
    products equals the integer one."""
    import numpy as np
    seed, rounds = int(seed), int(rounds)
    if not 0 <= seed <= _M32 or not 1 <= rounds <= SELFTEST_MAX_ROUNDS:
        raise ValueError("seed is 32 bits, rounds 1..1024")
    r = np.arange(rounds, dtype=np.uint64).reshape(-1, 1, 1)
    idx = np.arange(32, dtype=np.uint64).reshape(1, -1, 1)

    def i8(ab):  # [round][row or column][k] as int64
        w = np.arange(8, dtype=np.uint64).reshape(1, 1, -1)
        words = _selftest_hash(((np.uint64(2) * r + np.uint64(ab)) * np.uint64(32) + idx) * np.uint64(8) + w, seed)
        if inject and ab == 0:
            words[0, 0, 0] ^= np.uint64(1)
        b = (words[..., None] >> (np.uint64(8) * np.arange(4, dtype=np.uint64))) & np.uint64(0xFF)
        return b.astype(np.uint8).view(np.int8).astype(np.int64).reshape(rounds, 32, 32)

    def f16(ab):
        h = np.arange(2, dtype=np.uint64).reshape(1, 1, -1)
        bits = _selftest_hash(np.uint64(0x10000) + ((np.uint64(2) * r + np.uint64(ab)) * np.uint64(32) + idx) * np.uint64(2) + h,
                              seed)
        e = (bits[..., None] >> (np.uint64(4) * np.arange(8, dtype=np.uint64))) & np.uint64(7)
        return e.astype(np.int64).reshape(rounds, 32, 16) - 4

    a, b = i8(0), i8(1)
    ci = np.zeros((32, 32), dtype=np.int64)
    for k in range(rounds):
        ci += a[k] @ b[k].T
        assert np.abs(ci).max() <= (k + 1) << 19
    assert np.abs(ci).max() < 1 << 29, "the i8 accumulator left the range the definition promises"

    a, b = f16(0), f16(1)
    assert a.min() >= -4 and a.max() <= 3 and b.min() >= -4 and b.max() <= 3
    cf = np.zeros((32, 32), dtype=np.int64)
    cf32 = np.zeros((32, 32), dtype=np.float32)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    for k in range(rounds):
        for j in range(16):  # one product at a time: every partial sum is checked
            cf += np.outer(a[k][:, j], b[k][:, j])
            cf32 += np.outer(a32[k][:, j], b32[k][:, j])
            assert np.abs(cf).max() < 1 << 24, "an f16 partial sum left the exact range of float32"
    assert np.array_equal(cf32.astype(np.int64), cf) and np.array_equal(cf32, cf.astype(np.float32)), \
        "the float32 accumulation of the f16 test differs from the integer one"
    return ci, cf


def selftest_reference(seed, rounds, inject=False):
    """The four words of the known-answer test in pure numpy (the definition of
    native/include/vgpu/selftest.h): a dict unit -> uint32 value, in SELFTEST_UNITS order."""
    import numpy as np
    ci, cf = selftest_accumulators(seed, rounds, inject)
    m32 = np.uint64(_M32)
    lane = np.arange(64, dtype=np.uint64)
    x = _selftest_hash(np.uint64(0x20000) + lane, int(seed))
    for step in range(16 * int(rounds)):
        x = (x * np.uint64(0x9E3779B1) + np.uint64(step)) & m32
        x ^= x >> np.uint64(15)
    valu = int(_selftest_mix(x + lane).sum()) & _M32
    arr = np.zeros(64, dtype=np.uint64)
    arr[(17 * np.arange(64) + 5) & 63] = x
    loaded = arr[np.arange(64) ^ 21]
    lds = int(_selftest_mix(loaded + ((lane * np.uint64(0x9E3779B9)) & m32)).sum()) & _M32
    return {"valu": valu, "lds": lds, "mfma_i8": _selftest_fold(ci), "mfma_f16": _selftest_fold(cf)}


def decode_selftest_location(code):
    """(xcc, se, sh, cu, simd) from a cu_selftest location word."""
    return decode_location(int(code) & 0xFFFF) + ((int(code) >> 16) & 0x3,)


def cu_selftest(nblocks=2048, rounds=64, seed=0x5E1F7E57, hold_us=300, inject=(), device=None):
    """Runs the known-answer test in every wave of ``nblocks`` four-wave workgroups, each wave
    holding its CU ``hold_us`` afterwards so that the grid spreads over the whole slice, and
    compares every wave's four words with :func:`selftest_reference`. ``inject`` lists up to
    64 workgroups whose wave 0 runs with a flipped input bit (it must then show in ``bad``).

    Returns ``waves``, ``cus`` (the set of (xcc, se, sh, cu) covered), ``simd_pairs`` (distinct
    (cu, simd) pairs) and ``bad``: ``{block, wave, location, units}`` for every wave whose
    words differ from the reference, ``units`` naming those that do."""
    import numpy as np
    import torch
    device = torch.device(device or "cuda")
    nblocks, inject = int(nblocks), sorted({int(b) for b in inject})
    if nblocks < 1 or len(inject) > 64 or (inject and not 0 <= inject[0] <= inject[-1] < nblocks):
        raise ValueError("nblocks >= 1 and at most 64 injected workgroups inside the grid")
    want = selftest_reference(seed, rounds)  # validates seed and rounds
    out = torch.zeros(nblocks * 32, dtype=torch.int32, device=device)
    bad = torch.tensor(inject, dtype=torch.int32, device=device) if inject else None
    rc = _k().vgpu_cu_selftest(C.c_void_p(out.data_ptr()), nblocks, int(seed), int(rounds), int(hold_us),
                               C.c_void_p(bad.data_ptr()) if inject else None, len(inject), _stream(torch, device))
    if rc != 0:
        raise RuntimeError(f"vgpu_cu_selftest launch failed ({rc})")
    torch.cuda.synchronize(device)  # `bad` must outlive the kernel
    rec = out.cpu().numpy().view(np.uint32).reshape(nblocks * 4, 8)
    ref = np.array([want[u] for u in SELFTEST_UNITS], dtype=np.uint32)
    differs = rec[:, 1:5] != ref
    wrong = []
    for w in np.flatnonzero(differs.any(axis=1) | (rec[:, 5:] != 0).any(axis=1)).tolist():
        wrong.append({"block": w // 4, "wave": w % 4, "location": decode_selftest_location(rec[w, 0]),
                      "units": [u for u, d in zip(SELFTEST_UNITS, differs[w]) if d]})
    locs = np.unique(rec[:, 0]).tolist()
    return {"waves": nblocks * 4, "cus": {decode_location(c & 0xFFFF) for c in locs}, "simd_pairs": len(locs),
            "bad": wrong}


# ---- the memory-system probe (native/include/vgpu/memprobe.h)

RING_A = 0x9E3779B1
RING_MIN_L, RING_MAX_L = 1, 25         # rings of 2**L slots of 128 bytes: 256 B .. 4 GiB
RING_SLOT_BYTES = 128
MAX_CHASE_BLOCKS = 4096
MAX_CHASE_LANES = 64
MAX_CHASE_STEPS = 1 << 18
MAX_STREAM_WAVES = 16384
MAX_STREAM_PASSES = 1 << 20
CHASE_RECORD = 8                       # end slot, location, d(s_memtime) lo, hi, d(s_memrealtime), 0, 0, 0
STREAM_RECORD = 8                      # passes, sum, location, d(s_memrealtime) lo, hi, 0, 0, 0


def _ring_args(L, seed):
    L, seed = int(L), int(seed)
    if not RING_MIN_L <= L <= RING_MAX_L:
        raise ValueError(f"L {L} outside {RING_MIN_L}..{RING_MAX_L}")
    if not 0 <= seed <= _M32:
        raise ValueError("seed is 32 bits")
    return L, seed


def _ring_c(seed):
    return int(_selftest_hash(0x30000, seed)) | 1


def ring_reference(L, seed):
    """The ``next`` table of the pointer-chase ring in pure numpy: element i is word 0 of slot i,
    ``(A * i + C) mod 2**L`` as uint32 (the definition of native/include/vgpu/memprobe.h)."""
    import numpy as np
    L, seed = _ring_args(L, seed)
    i = np.arange(1 << L, dtype=np.uint64)
    return ((i * np.uint64(RING_A) + np.uint64(_ring_c(seed))) & np.uint64((1 << L) - 1)).astype(np.uint32)


def ring_jump(i, k, L, seed):
    """The slot reached from slot ``i`` after ``k`` steps (``k`` is taken mod 2**64, which the
    cycle's length divides): the affine map composed by squaring, as vgpu_ring_jump_slot. ``i``
    and ``k`` may be numpy arrays (``k`` then uint64); scalars give a Python int."""
    import numpy as np
    L, seed = _ring_args(L, seed)
    m32 = np.uint64(_M32)
    scalar = np.ndim(i) == 0 and np.ndim(k) == 0
    k = np.atleast_1d(np.asarray(k if np.ndim(k) else int(k) & (1 << 64) - 1, dtype=np.uint64)).copy()
    i = np.asarray(i, dtype=np.uint64) & m32
    ra, rc = np.ones_like(k), np.zeros_like(k)
    pa, pc = np.uint64(RING_A), np.uint64(_ring_c(seed))
    for _ in range(64):
        odd = (k & np.uint64(1)).astype(bool)
        rc = np.where(odd, (pa * rc + pc) & m32, rc)
        ra = np.where(odd, (pa * ra) & m32, ra)
        pc = (pa * pc + pc) & m32
        pa = (pa * pa) & m32
        k >>= np.uint64(1)
    at = ((ra * i + rc) & np.uint64((1 << L) - 1)).astype(np.uint32)
    return int(at[0]) if scalar else at


def _probe_tensor(t, what, align, min_bytes):
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous():
        raise ValueError(f"{what} needs a contiguous tensor")
    if t.data_ptr() % align:
        raise ValueError(f"{what} needs a {align}-byte aligned tensor")
    if nbytes < min_bytes:
        raise ValueError(f"{what} needs a tensor of at least {min_bytes} bytes")
    if not t.is_cuda:
        raise ValueError(f"{what} needs a CUDA tensor")
    return nbytes


def ring_build(t, L, seed):
    """Writes the ring of ``2**L`` slots into tensor ``t`` (asynchronous): words 0 and 1 of every
    128-byte slot, nothing else. ``t`` is a contiguous CUDA tensor, 128-byte aligned, of at
    least ``128 << L`` bytes; ``L`` in 1..25. Anything else is a ValueError."""
    import torch
    L, seed = _ring_args(L, seed)
    _probe_tensor(t, "ring_build", RING_SLOT_BYTES, RING_SLOT_BYTES << L)
    rc = _k().vgpu_ring_build(C.c_void_p(t.data_ptr()), L, seed, _stream(torch, t.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_ring_build launch failed ({rc})")


def mem_chase(ring, L, seed, nblocks, lanes, steps, first=0, chain_base=0, check=True, out=None):
    """Pointer chase over a built ring: ``nblocks`` (1..4096) single-wave workgroups whose lanes
    ``l < lanes`` (1..64) each make ``steps`` (1..2**18) dependent loads. Lane l of block b is
    chain ``g = chain_base + 64 * b + l`` and starts ``g * steps`` steps after slot ``first``, so
    consecutive chains tile the cycle, and a later launch with a larger ``chain_base`` touches
    fresh lines. Synchronises.

    Returns ``records`` (uint32 [nblocks * 64, 8]: end slot, location with SIMD, the s_memtime
    difference lo and hi, the s_memrealtime difference in 10 ns ticks, three zeros; rows of lanes
    >= ``lanes`` are not written), ``expected`` (uint32 [nblocks, lanes], every chain's end from
    :func:`ring_jump`), ``cycles`` and ``ticks`` ([nblocks, lanes]) and ``wall_s``, the host's
    clock around launch and synchronize. Unless ``check`` is false, a chain whose end differs
    raises RuntimeError naming it. ``out`` may give the int32 CUDA tensor of ``nblocks * 512``
    elements that the kernel writes."""
    import time
    import numpy as np
    import torch
    L, seed = _ring_args(L, seed)
    nblocks, lanes, steps, first, chain_base = int(nblocks), int(lanes), int(steps), int(first), int(chain_base)
    if not 1 <= nblocks <= MAX_CHASE_BLOCKS:
        raise ValueError(f"nblocks {nblocks} outside 1..{MAX_CHASE_BLOCKS}")
    if not 1 <= lanes <= MAX_CHASE_LANES:
        raise ValueError(f"lanes {lanes} outside 1..{MAX_CHASE_LANES}")
    if not 1 <= steps <= MAX_CHASE_STEPS:
        raise ValueError(f"steps {steps} outside 1..{MAX_CHASE_STEPS}")
    if not 0 <= first < 1 << L:
        raise ValueError(f"first {first} outside the ring")
    if not 0 <= chain_base < 1 << 64:
        raise ValueError("chain_base is 64 bits")
    _probe_tensor(ring, "mem_chase", RING_SLOT_BYTES, RING_SLOT_BYTES << L)
    words = nblocks * 64 * CHASE_RECORD
    if out is None:
        out = torch.zeros(words, dtype=torch.int32, device=ring.device)
    elif out.dtype != torch.int32 or out.numel() != words or out.device != ring.device:
        raise ValueError(f"out is an int32 tensor of {words} elements on the ring's device")
    else:
        _probe_tensor(out, "mem_chase", 4, 4 * words)
    torch.cuda.synchronize(ring.device)
    t0 = time.perf_counter()
    rc = _k().vgpu_mem_chase(C.c_void_p(ring.data_ptr()), L, seed, nblocks, lanes, steps, first, chain_base,
                             C.c_void_p(out.data_ptr()), _stream(torch, ring.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_mem_chase launch failed ({rc})")
    torch.cuda.synchronize(ring.device)
    wall = time.perf_counter() - t0
    rec = out.cpu().numpy().view(np.uint32).reshape(nblocks * 64, CHASE_RECORD)
    g = (np.uint64(chain_base) + np.arange(nblocks * 64, dtype=np.uint64).reshape(nblocks, 64)[:, :lanes])
    with np.errstate(over="ignore"):
        k = (g + np.uint64(1)) * np.uint64(steps)        # wraps mod 2**64, as the kernel's product does
    expected = ring_jump(first, k.reshape(-1), L, seed).reshape(nblocks, lanes)
    used = rec.reshape(nblocks, 64, CHASE_RECORD)[:, :lanes]
    if check:
        bad = np.argwhere(used[:, :, 0] != expected)
        if len(bad):
            b, l = (int(x) for x in bad[0])
            raise RuntimeError(f"mem_chase: chain {chain_base + 64 * b + l} (block {b}, lane {l}) ended at slot "
                               f"{int(used[b, l, 0])}, expected {int(expected[b, l])}; {len(bad)} chains differ")
    cycles = used[:, :, 2].astype(np.uint64) | used[:, :, 3].astype(np.uint64) << np.uint64(32)
    return {"records": rec, "expected": expected, "cycles": cycles, "ticks": used[:, :, 4].astype(np.uint64),
            "wall_s": wall}


def chase_steps(n, nblocks, warm):
    """The steps :func:`mem_latency` gives every chain of a one-lane launch over a ring of ``n``
    slots. With one lane, block b is chain ``64 * b`` and starts ``64 * b * steps`` slots along the
    cycle, so a power-of-two ``steps >= n / 64`` would start every chain at the same slot.

    * cold: ``n / (64 * nblocks)``: the chains lie ``n / nblocks`` apart, each walks the first
      64th of its stretch, and ``chain_base`` 1..63 walk the others.
    * warm, up to 2**18 slots: ``n``, every chain walks the whole ring.
    * warm, above: ``steps = t * n / 64 + d / 64`` with ``d = n / nblocks`` (down to a multiple of
      64) and ``t = ceil(64 / nblocks)``: then ``64 * steps = d (mod n)``, the chains start ``d``
      apart and each walks at least ``d`` slots, so together they cover the ring.

    At least 1024 (a few hundred microseconds) and at most 2**18."""
    n, nblocks = int(n), int(nblocks)
    if not warm:
        steps = n // (64 * nblocks)
    elif n <= MAX_CHASE_STEPS:
        steps = n
    else:
        steps = -(-64 // nblocks) * (n // 64) + (n // nblocks // 64 * 64) // 64
    return min(max(steps, 1024), MAX_CHASE_STEPS)


def mem_latency(nbytes, steps=None, nblocks=None, lanes=1, warm=None, seed=0x3E3F20BE, chain_base=0, ring=None,
                device=None):
    """Load-to-use latency over a working set of ``nbytes`` (a power of two, 256 B .. 4 GiB):
    allocates and builds the ring (or takes a built ``ring`` of that size and seed), makes one
    identical untimed launch when ``warm``, then the timed one.

    ``nblocks`` defaults to the CUs the device reports (one wave per CU of a slice) and ``steps``
    to :func:`chase_steps`: a warm launch covers the whole ring, a cold one walks every line
    once. ``warm`` defaults to true up to 256 MiB, the size of the Infinity Cache, and
    to false above: there a warm launch would only leave the few lines it touched in the caches,
    and the figure would be theirs. A cold launch with the next ``chain_base`` (add 1, up to 63,
    with one lane) walks lines that no earlier one has touched.

    Returns ``ns_per_load`` and ``cycles_per_load`` as ``{median, p10, p90}`` over the chains,
    ``cus`` (the set of (xcc, se, sh, cu) the waves ran on), ``chains``, ``steps``, ``warm`` and
    ``laps = steps / n``."""
    import numpy as np
    import torch
    nbytes = int(nbytes)
    L = nbytes.bit_length() - 1 - 7
    if nbytes != RING_SLOT_BYTES << max(L, 0) or not RING_MIN_L <= L <= RING_MAX_L:
        raise ValueError("the working set is a power of two between 256 bytes and 4 GiB")
    device = torch.device(device or (ring.device if ring is not None else "cuda"))
    if nblocks is None:
        nblocks = min(torch.cuda.get_device_properties(device).multi_processor_count, MAX_CHASE_BLOCKS)
    n = 1 << L
    if warm is None:
        warm = nbytes <= 256 << 20
    if steps is None:
        steps = chase_steps(n, nblocks, warm)
    if ring is None:
        ring = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
        ring_build(ring, L, seed)
    if warm:
        mem_chase(ring, L, seed, nblocks, lanes, steps, chain_base=chain_base)
    r = mem_chase(ring, L, seed, nblocks, lanes, steps, chain_base=chain_base)

    def spread(x):
        return {"median": float(np.median(x)), "p10": float(np.percentile(x, 10)), "p90": float(np.percentile(x, 90))}

    locs = np.unique(r["records"].reshape(int(nblocks), 64, CHASE_RECORD)[:, :int(lanes), 1])
    return {"bytes": nbytes, "L": L, "chains": int(nblocks) * int(lanes), "steps": int(steps), "laps": int(steps) / n,
            "warm": bool(warm),
            "ns_per_load": spread(r["ticks"].astype(np.float64) * 10.0 / steps),
            "cycles_per_load": spread(r["cycles"].astype(np.float64) / steps),
            "cus": {decode_location(int(c) & 0xFFFF) for c in locs}, "wall_s": r["wall_s"]}


def stream_chunks(n_vec, waves):
    """(begin, length) of every wave's chunk, in 16-byte vectors: ``n_vec // waves`` each and
    the first ``n_vec % waves`` waves one more."""
    import numpy as np
    q, r = divmod(int(n_vec), int(waves))
    w = np.arange(int(waves), dtype=np.int64)
    return w * q + np.minimum(w, r), q + (w < r).astype(np.int64)


def mem_stream(t, mode, waves, duration_us, max_passes, seed, base=0, check=True, out=None):
    """A controlled memory load for a fixed time: ``waves`` (1..16384, a multiple of 4) waves
    sweep tensor ``t`` (at least ``waves`` 16-byte vectors), each its own contiguous chunk, pass
    after pass for ``duration_us`` (0..1000000; 0 is exactly one pass) or ``max_passes``
    (1..2**20) passes. ``mode`` 0 (or "read") reads with non-temporal loads, 1 (or "write") writes
    the pattern of ``(base, seed)`` with non-temporal stores. Synchronises.

    Returns ``passes`` and ``ticks`` per wave, ``bytes`` moved in all, ``wall_s`` and ``gbps``
    over the host's clock around launch and synchronize, ``records`` (uint32 [waves, 8]) and
    ``cus``. With ``check``, read mode expects ``t`` to hold :func:`pattern_fill` of ``(seed,
    base)`` and verifies every wave's sum against ``passes * chunk_sum`` from
    :func:`pattern_reference`, write mode verifies the buffer with :func:`pattern_check`; a
    failure raises RuntimeError naming the wave (or the word)."""
    import time
    import numpy as np
    import torch
    mode = {"read": 0, "write": 1}.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError("mode is 0 / 'read' or 1 / 'write'")
    waves, duration_us, max_passes, seed, base = int(waves), int(duration_us), int(max_passes), int(seed), int(base)
    if not 1 <= waves <= MAX_STREAM_WAVES or waves % 4:
        raise ValueError(f"waves {waves} outside 1..{MAX_STREAM_WAVES} or no multiple of 4")
    if not 0 <= duration_us <= MAX_SPIN_US:
        raise ValueError(f"duration_us {duration_us} outside 0..{MAX_SPIN_US}")
    if not 1 <= max_passes <= MAX_STREAM_PASSES:
        raise ValueError(f"max_passes {max_passes} outside 1..{MAX_STREAM_PASSES}")
    if not 0 <= seed <= _M32 or not 0 <= base < 1 << 64:
        raise ValueError("seed is 32 bits, base 64")
    nbytes = t.numel() * t.element_size()
    if nbytes % 16:
        raise ValueError("mem_stream needs a multiple of 16 bytes")
    n_vec = nbytes // 16
    if n_vec < waves:
        raise ValueError(f"mem_stream needs at least one 16-byte vector per wave: n_vec {n_vec} < waves {waves}")
    _probe_tensor(t, "mem_stream", 16, 16)
    words = waves * STREAM_RECORD
    if out is None:
        out = torch.zeros(words, dtype=torch.int32, device=t.device)
    elif out.dtype != torch.int32 or out.numel() != words or out.device != t.device:
        raise ValueError(f"out is an int32 tensor of {words} elements on the buffer's device")
    else:
        _probe_tensor(out, "mem_stream", 16, 4 * words)
    torch.cuda.synchronize(t.device)
    t0 = time.perf_counter()
    rc = _k().vgpu_mem_stream(C.c_void_p(t.data_ptr()), n_vec, mode, waves, duration_us, max_passes, base, seed,
                              C.c_void_p(out.data_ptr()), _stream(torch, t.device))
    if rc != 0:
        raise RuntimeError(f"vgpu_mem_stream launch failed ({rc})")
    torch.cuda.synchronize(t.device)
    wall = time.perf_counter() - t0
    rec = out.cpu().numpy().view(np.uint32).reshape(waves, STREAM_RECORD)
    passes = rec[:, 0].astype(np.int64)
    begin, length = stream_chunks(n_vec, waves)
    if check and mode == 0:
        ref = pattern_reference(4 * n_vec, seed, base).astype(np.uint64)
        chunk = np.add.reduceat(ref, 4 * begin) & np.uint64(_M32)
        want = (chunk * passes.astype(np.uint64)) & np.uint64(_M32)
        bad = np.flatnonzero(rec[:, 1] != want)
        if len(bad):
            w = int(bad[0])
            raise RuntimeError(f"mem_stream: wave {w} summed {int(rec[w, 1]):#x} over {int(passes[w])} passes of vectors "
                               f"{int(begin[w])}..{int(begin[w] + length[w])}, expected {int(want[w]):#x}; "
                               f"{len(bad)} waves differ")
    if check and mode == 1:
        mismatches, first = pattern_check(t, seed, base)
        if mismatches:
            raise RuntimeError(f"mem_stream: {mismatches} words differ from the pattern after a write, the first is "
                               f"word {first}")
    total = int((passes * length).sum()) * 16
    ticks = rec[:, 3].astype(np.uint64) | rec[:, 4].astype(np.uint64) << np.uint64(32)
    return {"passes": passes, "ticks": ticks, "bytes": total, "wall_s": wall, "gbps": total / wall / 1e9,
            "records": rec, "cus": {decode_location(int(c) & 0xFFFF) for c in np.unique(rec[:, 2])}}
