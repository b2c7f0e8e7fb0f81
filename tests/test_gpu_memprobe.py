"""The memory probe (native/src/kernels/vgpu_kernels.hip: ring_build, mem_chase, mem_stream) on a
real MI355X, against the host references: exact equality for what a kernel writes, derived
bounds for what it times. No test asserts a latency tier or a bandwidth.

One child process, native (no contract, no preload), computes everything once; the tests assert
on what it reports. Every buffer a kernel writes sits between two 64-word guards of 0xA5A5A5A5.
Every call here has arguments the entry points accept: what they refuse is tested without a GPU
(tests/test_memprobe_args.py), so that a broken check cannot start a kernel here.

The timing bounds, and where they come from:

* s_memrealtime counts at 100 MHz, so its difference times 10 ns is time that passed inside the
  kernel, which the host's clock around launch and synchronize brackets: ticks * 10 ns <= wall *
  (1 + 1e-3), the 1e-3 an order above any crystal's tolerance.
* s_memtime counts shader cycles, and the shader clock never exceeds the maximum the device
  reports: d(s_memtime) / d(s_memrealtime) * 100 MHz <= clock_rate * (1 + 1e-3). The two stamps of
  a pair are read back to back at either end, so their offset cancels; what remains is one tick
  of quantisation in d(s_memrealtime). The cases are 2**16 and 2**18 dependent loads: no load
  returns in less than 10 ns, so the difference is above 65536 ticks and a tick of it below 2e-5.
* A stream of duration_us = 20000 leaves its pass loop only when 2 000 000 ticks have passed or
  max_passes are done, and stamps its end after that.
"""
import pytest

from conftest import run_child

pytestmark = pytest.mark.gpu

BUILD_L = [1, 2, 6, 8, 9, 13, 21]                       # 21: 2**21 slots, past the 4096 x 256 grid
CHASE_L = [1, 6, 13]
CHASE_STEPS = [1, 2, 1000]                              # 1000 > n at L = 1 and 6 (the chain wraps)
CHASE_LANES = [1, 2, 63, 64]
CHASE_BLOCKS = [1, 2, 300]
CHASE_BASES = [0, 1 << 40]                              # 2**40: the product g * steps needs 64 bits
TIMED = [(6, 1 << 16, 1), (13, 1 << 16, 64), (13, 1 << 18, 1)]   # L, steps, lanes
STREAM_SHAPES = [(4, 4), (5, 4), (4 * 63, 4), (4 * 64, 4), (4 * 65, 4), (4 * 257, 4), (1200 * 3 + 1, 1200)]
STREAM_RUNS = {"once": (0, 1 << 20), "three": (1000000, 3), "timed": (20000, 1 << 20)}   # duration_us, max_passes
SEED = 0x0DDBA11

CHILD = """
import ctypes
import numpy as np, torch
from amdvgpu.ops import (cu_census, mem_chase, mem_stream, pattern_check, pattern_fill, pattern_poke,
                         pattern_reference, ring_build, ring_jump, ring_reference)
from amdvgpu.ops.calib import _k, stream_chunks
GUARD, G, PRE = 64, 0xA5A5A5A5, 0x5C5C5C5C
BUILD_L, CHASE_L, CHASE_STEPS, CHASE_LANES, CHASE_BLOCKS, CHASE_BASES, TIMED, STREAM_SHAPES, STREAM_RUNS, SEED = %r
M32 = 0xFFFFFFFF

def s32(x):
    return x - (1 << 32) if x >> 31 else x

def u32(t):
    return t.cpu().numpy().view(np.uint32)

def guarded(n_words, fill=PRE):
    whole = torch.full((2 * GUARD + n_words,), s32(G), dtype=torch.int32, device="cuda")
    inner = whole[GUARD:GUARD + n_words]
    inner.fill_(s32(fill))
    return whole, inner

def guards(whole):
    return bool((whole[:GUARD] == s32(G)).all().item() and (whole[-GUARD:] == s32(G)).all().item())

def upload(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()

census = {c[0] << 12 | c[1] << 8 | c[2] << 4 | c[3] for c in cu_census(8192, 300)}

# ---- ring_build: words 0 and 1 of every slot, nothing else
builds, rings = {}, {}
for L in BUILD_L:
    n = 1 << L
    whole, ring = guarded(32 * n)
    ring_build(ring, L, SEED + L)
    torch.cuda.synchronize()
    v = ring.view(n, 32)
    builds[str(L)] = dict(
        word0=bool((v[:, 0] == upload(ring_reference(L, SEED + L))).all().item()),
        word1=bool((v[:, 1] == upload(np.arange(n, dtype=np.uint32) ^ np.uint32(SEED + L))).all().item()),
        rest=bool((v[:, 2:] == s32(PRE)).all().item()), guards=guards(whole))
    if L in CHASE_L:
        rings[L] = (whole, ring)
    else:
        del whole, ring, v

# ---- mem_chase: every chain's end slot, and what the kernel leaves alone
chases, slowest = {}, 0.0
for L in CHASE_L:
    n, seed, ring = 1 << L, SEED + L, rings[L][1]
    for steps in CHASE_STEPS:
        bad, cases = [], 0
        for lanes in CHASE_LANES:
            for nb in CHASE_BLOCKS:
                for first in (0, n - 1):
                    for base in CHASE_BASES:
                        whole, out = guarded(nb * 512)
                        r = mem_chase(ring, L, seed, nb, lanes, steps, first=first, chain_base=base, check=False, out=out)
                        rec = r["records"].reshape(nb, 64, 8)
                        used, unused = rec[:, :lanes], rec[:, lanes:]
                        ok = dict(ends=bool(np.array_equal(used[:, :, 0], r["expected"])),
                                  unused=bool((unused == PRE).all()), zeros=bool((used[:, :, 5:] == 0).all()),
                                  guards=guards(whole), ring=guards(rings[L][0]),
                                  location=all(int(c) & 0xFFFF in census and int(c) >> 18 == 0 for c in np.unique(used[:, :, 1])),
                                  positive=bool((r["cycles"] > 0).all() and (r["ticks"] > 0).all()),
                                  wall=bool(float(r["ticks"].max()) * 1e-8 <= r["wall_s"] * (1 + 1e-3)))
                        cases += 1
                        slowest = max(slowest, r["wall_s"])
                        if not all(ok.values()):
                            bad.append(dict(lanes=lanes, nblocks=nb, first=first, chain_base=base,
                                            failed=[k for k, v in ok.items() if not v]))
        chases["%%d-%%d" %% (L, steps)] = dict(cases=cases, bad=bad[:8])
    # the expected ends themselves, once per ring, against a walk of the reference table
    ref = ring_reference(L, seed)
    r = mem_chase(ring, L, seed, 2, 64, 2, first=n - 1)
    at, walk = n - 1, []
    for g in range(129):
        walk.append(at)
        at = int(ref[int(ref[at])])
    chases["walk-%%d" %% L] = bool(r["expected"].reshape(-1).tolist() == walk[1:])

# ---- mem_chase: the two clocks
khz = ctypes.c_int(0)
rc = _k().hipDeviceGetAttribute(ctypes.byref(khz), 5, 0)    # hipDeviceAttributeClockRate: the maximum, in kHz
clock_khz = khz.value if rc == 0 else 0
timed = []
for L, steps, lanes in TIMED:
    r = mem_chase(rings[L][1], L, SEED + L, 2, lanes, steps)
    timed.append(dict(L=L, steps=steps, lanes=lanes, cycles=r["cycles"].reshape(-1).tolist(),
                      ticks=r["ticks"].reshape(-1).tolist(), wall_s=r["wall_s"]))

# ---- mem_chase must be able to fail: word 0 of a slot that chain 0 visits
whole, ring = rings[6]
slot = ring_jump(0, 3, 6, SEED + 6)
ring.view(64, 32)[slot, 0] = (int(ring_reference(6, SEED + 6)[slot]) + 1) & 63
try:
    mem_chase(ring, 6, SEED + 6, 1, 1, 10)
    chase_fails = "no error"
except RuntimeError as e:
    chase_fails = str(e)

# ---- mem_stream
BASE = (1 << 33) + 6
def chunk_sums(n_vec, waves, seed):
    ref = pattern_reference(4 * n_vec, seed, BASE)
    begin, length = stream_chunks(n_vec, waves)
    return ref, [int(ref[4 * b:4 * (b + l)].astype(np.uint64).sum()) & M32 for b, l in zip(begin.tolist(), length.tolist())]

def timing(r, max_passes):
    return dict(passes=r["passes"].tolist(), ticks=r["ticks"].tolist(), wall_s=r["wall_s"], max_passes=max_passes)

streams = {}
for n_vec, waves in STREAM_SHAPES:
    seed = SEED ^ n_vec
    ref, sums = chunk_sums(n_vec, waves, seed)
    src = torch.empty(4 * n_vec, dtype=torch.int32, device="cuda")
    pattern_fill(src, seed, BASE)
    for name, (us, max_passes) in STREAM_RUNS.items():
        whole, out = guarded(8 * waves)
        r = mem_stream(src, "read", waves, us, max_passes, seed, base=BASE, out=out)
        rec = r["records"]
        streams["read-%%d-%%d-%%s" %% (n_vec, waves, name)] = dict(
            timing(r, max_passes), guards=guards(whole), zeros=bool((rec[:, 5:] == 0).all()),
            sums=all(int(rec[w, 1]) == sums[w] * int(rec[w, 0]) & M32 for w in range(waves)),
            source=bool(np.array_equal(u32(src), ref)),
            location=all(int(c) & 0xFFFF in census for c in np.unique(rec[:, 2])))
        old = pattern_reference(4 * n_vec, seed + 1, BASE)
        whole_b, buf = guarded(4 * n_vec)
        buf.copy_(upload(old))
        whole, out = guarded(8 * waves)
        r = mem_stream(buf, "write", waves, us, max_passes, seed, base=BASE, out=out)
        rec, got = r["records"], u32(buf)
        streams["write-%%d-%%d-%%s" %% (n_vec, waves, name)] = dict(
            timing(r, max_passes), guards=guards(whole) and guards(whole_b), zeros=bool((rec[:, 5:] == 0).all()),
            sums=bool((rec[:, 1] == 0).all()), check=list(pattern_check(buf, seed, BASE)),
            equal=bool(np.array_equal(got, ref)), old_words=int((got == old).sum()), expected_old=int((ref == old).sum()))

# ---- mem_stream must be able to fail: one word of wave 2's chunk (vectors 130..195 of 260)
n_vec, waves, seed = 260, 4, SEED ^ 260
src = torch.empty(4 * n_vec, dtype=torch.int32, device="cuda")
pattern_fill(src, seed, BASE)
pattern_poke(src, [4 * 130 + 5])
try:
    mem_stream(src, "read", waves, 0, 1, seed, base=BASE)
    stream_fails = "no error"
except RuntimeError as e:
    stream_fails = str(e)

emit(builds=builds, chases=chases, slowest_chase_s=slowest, clock_khz=clock_khz, timed=timed, chase_fails=chase_fails,
     streams=streams, stream_fails=stream_fails, census=len(census))
""" % ((BUILD_L, CHASE_L, CHASE_STEPS, CHASE_LANES, CHASE_BLOCKS, CHASE_BASES, TIMED, STREAM_SHAPES, STREAM_RUNS, SEED),)


@pytest.fixture(scope="module")
def results():
    res, _ = run_child(CHILD, None, timeout=300)
    return res[0]


@pytest.mark.parametrize("L", BUILD_L)
def test_ring_build_equals_the_reference(results, L):
    r = results["builds"][str(L)]
    assert r["word0"], "word 0 of a slot differs from ring_reference"
    assert r["word1"], "word 1 of a slot is not slot ^ seed"
    assert r["rest"], "a word 2..31 of a slot was written"
    assert r["guards"], "a word outside the ring was written"


@pytest.mark.parametrize("steps", CHASE_STEPS)
@pytest.mark.parametrize("L", CHASE_L)
def test_mem_chase_ends_where_the_reference_does(results, L, steps):
    """Every chain of every launch: lanes 1, 2, 63, 64 x nblocks 1, 2, 300 x first 0, n - 1 x
    chain_base 0, 2**40. Besides the end slots: records of lanes >= `lanes` keep their prefill,
    words 5..7 are zero, guards of the records and of the ring are whole, the location is a CU
    of the census, both clocks advanced, and the 100 MHz clock stays inside the host's."""
    r = results["chases"][f"{L}-{steps}"]
    assert r["cases"] == len(CHASE_LANES) * len(CHASE_BLOCKS) * 2 * len(CHASE_BASES)
    assert not r["bad"], r["bad"]


@pytest.mark.parametrize("L", CHASE_L)
def test_mem_chase_expected_ends_equal_a_walk(results, L):
    """The ends the launches are compared with, from ring_jump, against walking ring_reference."""
    assert results["chases"][f"walk-{L}"]
    assert results["slowest_chase_s"] < 1.0


@pytest.mark.parametrize("case", range(len(TIMED)), ids=[f"L{L}-steps{s}-lanes{l}" for L, s, l in TIMED])
def test_mem_chase_clocks_stay_inside_their_bounds(results, case):
    """Both differences above 0, the 100 MHz clock inside the host's wall time, and the shader
    clock, d(s_memtime) / d(s_memrealtime) * 100 MHz, at most the maximum the device reports
    (hipDeviceAttributeClockRate) times (1 + 1e-3).

    The last bound holds in some runs on the MI355X and is missed in others, by the same 0.23-0.25 %
    in every case of such a run. The device reports 2 400 000 kHz; two runs gave 2391-2397 MHz
    (144.1 cycles / 60.2 ns, 230.5 / 96.4, 240.8 / 100.7 per load) and passed, two others gave
        L=6  steps=2**16 lanes=1:   9 837 372 cycles /   408 856 ticks = 2406.1 MHz
                                    9 885 184        /   410 956       = 2405.4 MHz (second run)
        L=13 steps=2**16 lanes=64: 14 680 116        /   610 200       = 2405.8 MHz
        L=13 steps=2**18 lanes=1:  61 472 820        / 2 555 500       = 2405.5 MHz
    and failed. The stamps of a pair are read in the same order at both ends and a tick of the
    100 MHz counter is below 3e-6 of these differences, so this is what the counters do on that
    machine - its shader clock in a latency-bound kernel runs 0.24 % above the nominal maximum, or
    its 100 MHz counter as much below - and not the kernel's doing.
    The bound stays as it was set; the cycles per load this probe reports are s_memtime's."""
    r, khz = results["timed"][case], results["clock_khz"]
    steps = r["steps"]
    print(f"L={r['L']} steps={steps} lanes={r['lanes']}: cycles/load {[round(c / steps, 1) for c in r['cycles'][:4]]}, "
          f"ns/load {[round(t * 10 / steps, 1) for t in r['ticks'][:4]]}, wall {r['wall_s'] * 1e3:.2f} ms, "
          f"max clock {khz / 1e3:.0f} MHz")
    assert len(r["cycles"]) == 2 * r["lanes"]
    assert 500e3 <= khz <= 5e6, "the device reports no plausible maximum clock"
    for cycles, ticks in zip(r["cycles"], r["ticks"]):
        assert cycles > 0 and ticks > 0
        assert ticks * 1e-8 <= r["wall_s"] * (1 + 1e-3)
        assert cycles / ticks * 1e8 <= khz * 1e3 * (1 + 1e-3)


def _stream(results, mode, shape, run):
    return results["streams"][f"{mode}-{shape[0]}-{shape[1]}-{run}"]


def _passes_and_time(r, run):
    duration_us, max_passes = STREAM_RUNS[run]
    if run == "once":
        assert set(r["passes"]) == {1}, "duration_us = 0 is exactly one pass"
    elif run == "three":
        assert set(r["passes"]) == {3}, "max_passes ends the loop"
    else:
        for passes, ticks in zip(r["passes"], r["ticks"]):
            assert 1 <= passes <= max_passes
            assert passes == max_passes or ticks >= duration_us * 100
    assert max(r["ticks"]) * 1e-8 <= r["wall_s"] * (1 + 1e-3)


@pytest.mark.parametrize("run", sorted(STREAM_RUNS))
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=[f"{n}-{w}" for n, w in STREAM_SHAPES])
def test_mem_stream_read(results, shape, run):
    r = _stream(results, "read", shape, run)
    _passes_and_time(r, run)
    assert r["sums"], "a wave's sum is not passes * chunk_sum from pattern_reference"
    assert r["source"], "the source changed"
    assert r["zeros"] and r["location"]
    assert r["guards"], "a word outside the records was written"


@pytest.mark.parametrize("run", sorted(STREAM_RUNS))
@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=[f"{n}-{w}" for n, w in STREAM_SHAPES])
def test_mem_stream_write(results, shape, run):
    r = _stream(results, "write", shape, run)
    _passes_and_time(r, run)
    assert r["check"] == [0, None], "pattern_check finds mismatches after the write"
    assert r["equal"], "the buffer differs from pattern_reference"
    assert r["old_words"] == r["expected_old"], "a word of the earlier fill is left"
    assert r["sums"] and r["zeros"]
    assert r["guards"], "a word outside the buffer or the records was written"


def test_both_checks_can_fail(results):
    """One poked word of wave 2's chunk, and one overwritten `next` of a slot chain 0 visits."""
    assert "wave 2" in results["stream_fails"], results["stream_fails"]
    assert "chain 0 " in results["chase_fails"], results["chase_fails"]
