"""The calibration kernels behind the README's numbers (native/src/kernels/vgpu_kernels.hip:
stream_copy, scratch_hog, spin, spin_lds, cu_census) on a real MI355X, each against a host
reference: exact equality for what a kernel writes, derived bounds for how long it runs.

One child process, native (no contract, no preload), computes everything once; the tests assert
on what it reports. Every buffer a kernel writes sits between two 64-word guards of 0xA5A5A5A5.
Every call here has arguments the entry points accept: what they refuse is tested without a GPU
(tests/test_calib_args.py), so that a broken check cannot start a kernel here.

Copy sizes, in 16-byte vectors: 1, around one wave (63-65), around one block (255-257) and one
past the grid cap (4096 blocks x 256 lanes), where the grid-stride loop takes a second turn.
"""
import statistics

import pytest

from conftest import run_child

pytestmark = pytest.mark.gpu

CAP = 4096 * 256
SIZES = [1, 63, 64, 65, 255, 256, 257, CAP + 1]
STRIDES = [1, 3, 4095, 0x7FFFFFFF, 506952113]          # the last is scratch_hog's default
BLOCKS = [1, 2, 300]
COUNTS = [1, 2, 300, 70000]                             # 70000: past 16 bits of grid index
SPIN_T = 20000                                          # us, the duration cases
LDS_T = 5000                                            # us, the residency cases
LDS_SIZES = [1, 64 << 10, 160 << 10]

# Margins of the duration test, in us (see its docstring for the figures behind them).
LOWER_MARGIN_US = 0.0
UPPER_MARGIN_US = 0.0

CHILD = """
import ctypes
import numpy as np, torch
from amdvgpu.ops import (cu_census, decode_location, pattern_reference, scratch_hog, scratch_reference, spin,
                         spin_lds, stream_copy)
from amdvgpu.ops.calib import _k
GUARD, G = 64, 0xA5A5A5A5
SIZES, STRIDES, BLOCKS, COUNTS, SPIN_T, LDS_T, LDS_SIZES = %r
P, L = ctypes.c_void_p, _k()
CUS = torch.cuda.get_device_properties(0).multi_processor_count

def u32(t):
    return t.cpu().numpy().view(np.uint32)

def guarded(n_words):
    whole = torch.full((2 * GUARD + n_words,), G - (1 << 32), dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + n_words]

def guards(whole):
    h = u32(whole)
    return bool((h[:GUARD] == G).all() and (h[-GUARD:] == G).all())

def upload(words):
    return torch.from_numpy(words.view(np.int32)).cuda()

def same(t, words):
    return bool(np.array_equal(u32(t), words))

# ---- stream_copy: every word of the source depends on its position
copies = {}
for n_vec in SIZES:
    ref = pattern_reference(4 * n_vec, 0x7000 + n_vec)
    src = upload(ref)
    whole, dst = guarded(4 * n_vec)
    stream_copy(dst, src)
    torch.cuda.synchronize()
    copies[str(n_vec)] = dict(equal=same(dst, ref), guards=guards(whole), source=same(src, ref))

new, old = pattern_reference(4 * 257, 0xA11CE), pattern_reference(4 * 257, 0xB0B)
src = upload(new)
whole, dst = guarded(4 * 257)
dst.copy_(upload(old))
stream_copy(dst, src, 16 * 65)
torch.cuda.synchronize()
h = u32(dst)
partial = dict(head=bool(np.array_equal(h[:4 * 65], new[:4 * 65])), tail=bool(np.array_equal(h[4 * 65:], old[4 * 65:])),
               guards=guards(whole), source=same(src, new))

dst.copy_(upload(old))
stream_copy(dst, src, 0)
rc = L.vgpu_stream_copy(P(dst.data_ptr()), P(src.data_ptr()), 0, None)
torch.cuda.synchronize()
zero = dict(rc=rc, untouched=same(dst, old), guards=guards(whole))

ref = pattern_reference(4 * 65, 0xD7)
src8 = torch.from_numpy(ref.view(np.uint8)).cuda()
whole, dst = guarded(4 * 65)
stream_copy(dst, src8)
torch.cuda.synchronize()
dtypes = dict(equal=same(dst, ref), guards=guards(whole), src=str(src8.dtype), dst=str(dst.dtype))

# ---- scratch_hog: the raw entry into a guarded buffer
refs = {s: scratch_reference(s) for s in STRIDES}
scratch = {}
for nb in BLOCKS:
    for s in STRIDES:
        whole, out = guarded(64 * nb)
        rc = L.vgpu_scratch_hog(P(out.data_ptr()), nb, s, None)
        torch.cuda.synchronize()
        got = u32(out).reshape(nb, 64)
        scratch["%%d-%%d" %% (nb, s)] = dict(rc=rc, equal=bool((got == refs[s]).all()), guards=guards(whole))
y = scratch_hog(nblocks=2)
torch.cuda.synchronize()
scratch_default = bool((u32(y).reshape(2, 64) == scratch_reference()).all())

# ---- spin: the done counter, an int64 between 32-element (64-word) guards
G64 = (G << 32 | G) - (1 << 64)
counts = {}
for nb in COUNTS:
    whole = torch.full((65,), G64, dtype=torch.int64, device="cuda")
    counter = whole[32:33]
    counter.zero_()
    spin(nb, 0, counter=counter)
    torch.cuda.synchronize()
    first = int(counter.item())
    spin(nb, 0, counter=counter)
    torch.cuda.synchronize()
    h = whole.cpu()
    counts[str(nb)] = dict(first=first, second=int(h[32]), guards=bool((h[:32] == G64).all() and (h[33:] == G64).all()))
spin(3, 0)
torch.cuda.synchronize()
no_counter = True

# ---- durations, in us, between two HIP events
def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0

spin(1, 1000)
torch.cuda.synchronize()
durations = {str(us): [timed(lambda: spin(1, us)) for _ in range(5)] for us in (0, SPIN_T, 2 * SPIN_T)}

# ---- spin_lds: does a size launch, and does the LDS it holds limit residency
lds_launch = {}
for nbytes in LDS_SIZES:
    rc = L.vgpu_spin_lds(1, 10, nbytes, None)
    torch.cuda.synchronize()
    lds_launch[str(nbytes)] = rc
residency = {}
for name, nbytes in (("big", 96 << 10), ("small", 1024)):
    try:
        spin_lds(1, 10, nbytes)                             # warm-up
        torch.cuda.synchronize()
        residency[name] = timed(lambda: spin_lds(2 * CUS, LDS_T, nbytes))
    except RuntimeError as e:
        residency[name] = str(e)

# ---- cu_census: the raw buffer, one code per block
full = cu_census(8192, 300)
census = {}
for nb in BLOCKS:
    whole, out = guarded(nb)
    rc = L.vgpu_cu_census(P(out.data_ptr()), nb, 10, None)
    torch.cuda.synchronize()
    codes = u32(out).tolist()
    census[str(nb)] = dict(rc=rc, n=len(codes), guards=guards(whole), high_bits=any(c >> 16 for c in codes),
                           members=all(decode_location(c) in full for c in codes))

emit(cus=CUS, copies=copies, partial=partial, zero=zero, dtypes=dtypes, scratch=scratch, scratch_default=scratch_default,
     counts=counts, no_counter=no_counter, durations=durations, lds_launch=lds_launch, residency=residency,
     census=census, census_full=len(full))
""" % ((SIZES, STRIDES, BLOCKS, COUNTS, SPIN_T, LDS_T, LDS_SIZES),)


@pytest.fixture(scope="module")
def results():
    res, _ = run_child(CHILD, None, timeout=180)
    return res[0]


@pytest.mark.parametrize("n_vec", SIZES)
def test_stream_copy_equals_the_source(results, n_vec):
    r = results["copies"][str(n_vec)]
    assert r["equal"], "a copied word differs from the source"
    assert r["guards"], "a word outside dst was written"
    assert r["source"], "the source changed"


def test_stream_copy_of_a_part_leaves_the_rest(results):
    """16 * 65 bytes into a 257-vector dst that holds another seed's pattern."""
    assert results["partial"] == {"head": True, "tail": True, "guards": True, "source": True}


def test_stream_copy_of_zero_bytes_writes_nothing(results):
    assert results["zero"] == {"rc": 0, "untouched": True, "guards": True}


def test_stream_copy_between_dtypes_of_equal_byte_size(results):
    assert results["dtypes"] == {"equal": True, "guards": True, "src": "torch.uint8", "dst": "torch.int32"}


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("nblocks", BLOCKS)
def test_scratch_hog_equals_the_reference(results, nblocks, stride):
    r = results["scratch"][f"{nblocks}-{stride}"]
    assert r["rc"] == 0
    assert r["equal"], "a block's 64 checksums differ from scratch_reference"
    assert r["guards"], "a word outside the buffer was written"


def test_scratch_hog_default_call(results):
    assert results["scratch_default"]


@pytest.mark.parametrize("nblocks", COUNTS)
def test_spin_counts_every_workgroup_once(results, nblocks):
    r = results["counts"][str(nblocks)]
    assert r["first"] == nblocks, r
    assert r["second"] == 2 * nblocks, r
    assert r["guards"], "a word next to the counter was written"


def test_spin_without_a_counter_completes(results):
    assert results["no_counter"]


def test_spin_lasts_what_it_is_asked(results):
    """One workgroup spinning T = 20000 us and one 2T, each between two HIP events, 5 times.

    Lower bound, every repeat: the kernel counts T on the 100 MHz clock and the events bracket
    it, so elapsed >= T (and >= 2T) less LOWER_MARGIN_US. Upper bound, the median of 5: elapsed(T)
    <= T + the median elapsed of the same launch with spin_us = 0, plus UPPER_MARGIN_US.

    Measured on an MI355X (profiles/calib/README.md), first run: elapsed(0) 17.3, 12.4, 11.9, 11.8,
    10.2 us; elapsed(T) 20007.0, 20009.6, 20008.1, 20007.3, 20006.9 us; elapsed(2T) 40008.0, 40011.0,
    40011.8, 40009.7, 40008.5 us. The event clock never read short of the kernel's (the least
    elapsed - T over nine runs of this file was 6.9 us), so LOWER_MARGIN_US is 0. The excess of
    elapsed(T) over T + median elapsed(0) was -4.9, -2.3, -3.7, -4.6, -4.9 us: a spinning launch
    costs about 7 us beside its spin, an empty one about 12 us between the same two events. The
    largest excess is negative (-2.3 us, and never above -2.9 us in the eight later runs), three
    times it is no margin, so UPPER_MARGIN_US is 0 as well.
    """
    d = {int(k): v for k, v in results["durations"].items()}
    base = statistics.median(d[0])
    for us in (0, SPIN_T, 2 * SPIN_T):
        print(f"spin_us={us}: elapsed {[round(x, 1) for x in d[us]]} us, over spin_us + median(0) "
              f"{[round(x - us - base, 1) for x in d[us]]} us")
    assert min(d[SPIN_T]) >= SPIN_T - LOWER_MARGIN_US
    assert min(d[2 * SPIN_T]) >= 2 * SPIN_T - LOWER_MARGIN_US
    assert statistics.median(d[SPIN_T]) <= SPIN_T + base + UPPER_MARGIN_US


@pytest.mark.parametrize("lds_bytes", LDS_SIZES)
def test_spin_lds_launches(results, lds_bytes):
    """1 byte, 64 KiB and a CU's whole 160 KiB of dynamic LDS: each launches and synchronises."""
    assert results["lds_launch"][str(lds_bytes)] == 0


def test_spin_lds_limits_residency(results):
    """2 * CUs single-wave workgroups spinning T = 5000 us each. With 96 KiB of LDS at most one
    fits a CU's 160 KiB, so the grid needs two rounds at least: elapsed >= 2T, derived. With
    1 KiB all are resident at once, and the same grid takes less than 2T."""
    big, small = results["residency"]["big"], results["residency"]["small"]
    print(f"{2 * results['cus']} workgroups of {LDS_T} us: {big} us holding 96 KiB, {small} us holding 1 KiB")
    assert isinstance(big, float) and isinstance(small, float), (big, small)
    assert big >= 2 * LDS_T
    assert small < 2 * LDS_T


@pytest.mark.parametrize("nblocks", BLOCKS)
def test_cu_census_writes_one_code_per_block(results, nblocks):
    r = results["census"][str(nblocks)]
    assert r["rc"] == 0 and r["n"] == nblocks
    assert r["guards"], "a word outside the buffer was written"
    assert not r["high_bits"], "a code has a bit above 15"
    assert r["members"], "a code names no CU of the full census"
    assert results["census_full"] == results["cus"]
