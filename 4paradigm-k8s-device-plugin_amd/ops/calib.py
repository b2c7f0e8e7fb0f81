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

The wrappers refuse with ValueError what the C entry points refuse with -1
(native/include/vgpu/calib_args.h): no spin longer than a second or negative, no grid past
2**20 workgroups, no copy of strided, misaligned, overlapping or host tensors.

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
