"""The pattern kernels (native/src/kernels/device_kernels.h, amdvgpu.ops.pattern_*) on a real
MI355X: integer results, exact equality with the numpy definition (pattern_reference, which
tests/test_validate_conformance.py pins to the C definition).

One child process computes everything once; the tests assert on what it reports.
Sizes, in 16-byte vectors: 1, around one wave (63-65), around one block (255-257) and one
past the grid cap (4096 blocks x 256 lanes), where the grid-stride loop takes a second turn.
"""
import pytest

from conftest import run_child

pytestmark = pytest.mark.gpu

CAP = 4096 * 256
SIZES = [1, 63, 64, 65, 255, 256, 257, CAP + 1]

CHILD = """
import ctypes
import numpy as np, torch
from amdvgpu.ops import pattern_fill, pattern_check, pattern_poke, pattern_reference
from amdvgpu.ops.calib import _k
GUARD, G = 64, 0xA5A5A5A5
SIZES = %r

def u32(t):
    return t.cpu().numpy().view(np.uint32)

def guarded(n_vec):
    whole = torch.full((2 * GUARD + 4 * n_vec,), G - (1 << 32), dtype=torch.int32, device="cuda")
    return whole, whole[GUARD:GUARD + 4 * n_vec]

def filled(n_vec, seed, base=0):
    whole, t = guarded(n_vec)
    pattern_fill(t, seed, base)
    torch.cuda.synchronize()
    h = u32(whole)
    ref = pattern_reference(4 * n_vec, seed, base)
    return t, dict(equal=bool(np.array_equal(h[GUARD:-GUARD], ref)),
                   guards=bool((h[:GUARD] == G).all() and (h[-GUARD:] == G).all()),
                   clean=pattern_check(t, seed, base))

fills = {}
for n_vec in SIZES:
    big, fills[str(n_vec)] = filled(n_vec, 0x9000 + n_vec)
seed_big, W = 0x9000 + SIZES[-1], 4 * SIZES[-1]

_, wrap = filled(256, 0xC0FFEE, base=2**32 - 64)          # 4 KiB across word index 2**32
_, odd = filled(65, 0xBEEF, base=3)                        # a base that starts no pattern vector

cases = {
    "first_and_last": [0, W - 1],
    "two_in_one_wave": [4 * 10 + 1, 4 * 40 + 2],
    "grid_stride_tail": [W - 3],
    "one_in_each_of_several_waves": [4 * (64 * k + 5) for k in range(1, 8)],
    "waves_of_several_blocks": [4 * (256 * k + 64 * (k %% 4) + 9) + 3 for k in (1, 2, 700, 4095)],
}
corrupt = {}
for name, idx in cases.items():
    pattern_poke(big, idx)
    got = pattern_check(big, seed_big)
    pattern_poke(big, idx)                                  # the same bit again: restored
    corrupt[name] = dict(idx=idx, got=got, restored=pattern_check(big, seed_big))

t, _ = filled(257, 41)
ref = pattern_reference(4 * 257, 41)
wrong = {}
for name, (seed, base) in {"seed": (42, 0), "base_aligned": (41, 4), "base_odd": (41, 1)}.items():
    diff = ref != pattern_reference(4 * 257, seed, base)     # on the host, from the reference alone
    wrong[name] = dict(got=pattern_check(t, seed, base), want=[int(diff.sum()), int(np.argmax(diff))])

def raises(fn):
    try:
        fn()
    except ValueError:
        return True
    return False
x = torch.zeros(6, dtype=torch.int32, device="cuda")          # 24 bytes
out = torch.tensor([0, -1], dtype=torch.int64, device="cuda")
P = ctypes.c_void_p
size = dict(fill=raises(lambda: pattern_fill(x, 1)), check=raises(lambda: pattern_check(x, 1)),
            poke=raises(lambda: pattern_poke(x, [6])),
            c_fill=_k().vgpu_pattern_fill(P(x.data_ptr()), 24, 0, 1, None),
            c_check=_k().vgpu_pattern_check(P(x.data_ptr()), 24, 0, 1, P(out.data_ptr()), None))
torch.cuda.synchronize()
emit(fills=fills, wrap=wrap, odd=odd, corrupt=corrupt, wrong=wrong, size=size, untouched=bool((x == 0).all()))
""" % (SIZES,)


@pytest.fixture(scope="module")
def results():
    res, _ = run_child(CHILD, None, timeout=120)
    return res[0]


@pytest.mark.parametrize("n_vec", SIZES)
def test_fill_equals_the_reference(results, n_vec):
    r = results["fills"][str(n_vec)]
    assert r["equal"], "a filled word differs from pattern_reference"
    assert r["guards"], "a word outside the buffer was written"
    assert r["clean"] == [0, None]


def test_fill_across_the_32_bit_word_index(results):
    """base = 2**32 - 64 words, a 4 KiB buffer: a 32-bit index would wrap to word 0's pattern."""
    assert results["wrap"] == {"equal": True, "guards": True, "clean": [0, None]}


def test_fill_from_an_unaligned_base(results):
    assert results["odd"] == {"equal": True, "guards": True, "clean": [0, None]}


@pytest.mark.parametrize("case", ["first_and_last", "two_in_one_wave", "grid_stride_tail",
                                  "one_in_each_of_several_waves", "waves_of_several_blocks"])
def test_check_counts_and_locates_corrupted_words(results, case):
    r = results["corrupt"][case]
    assert r["got"] == [len(r["idx"]), min(r["idx"])], r
    assert r["restored"] == [0, None]


@pytest.mark.parametrize("what", ["seed", "base_aligned", "base_odd"])
def test_check_against_a_wrong_seed_or_base(results, what):
    r = results["wrong"][what]
    assert r["want"][0] > 1000            # nearly every word of the 1028 differs
    assert r["got"] == r["want"], r


def test_a_size_that_is_no_multiple_of_16_raises(results):
    s = results["size"]
    assert s["fill"] and s["check"] and s["poke"]
    assert s["c_fill"] == -1 and s["c_check"] == -1
    assert results["untouched"]
