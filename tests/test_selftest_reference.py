"""The known-answer test of the compute conformance check on the CPU: the numpy definition
(amdvgpu.ops.selftest_reference) against the tool's host C (native/include/vgpu/selftest.h,
which the gfx950 kernel cu_selftest and the fake runtime share), and the properties that the
definition promises about its own arithmetic.
"""
import os
import subprocess

import numpy as np
import pytest

from amdvgpu.ops import selftest_reference
from amdvgpu.ops.calib import SELFTEST_UNITS, selftest_accumulators
from amdvgpu.shim.native import VALIDATE, lib_path

SEEDS = [1, 0x5EED0001, 0xFFFFFFFF]
ROUNDS = [1, 2, 64, 1024]


def tool(*args, env=None):
    return subprocess.run([lib_path(VALIDATE), *args], env=env, capture_output=True, text=True, timeout=120)


def expected(seed, rounds, inject=False):
    p = tool("--selftest-expected", str(seed), str(rounds), *(["inject"] if inject else []))
    assert p.returncode == 0, p.stderr
    lines = [l.split() for l in p.stdout.splitlines()]
    assert [l[0] for l in lines] == list(SELFTEST_UNITS)
    return {l[0]: int(l[1]) for l in lines}


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_equals_the_host_definition(seed, rounds):
    want = expected(seed, rounds)
    got = selftest_reference(seed, rounds)
    assert list(got) == list(SELFTEST_UNITS) and all(0 <= v < 1 << 32 for v in got.values())
    assert got == want
    assert selftest_reference(seed, rounds, inject=True) == expected(seed, rounds, inject=True)


def test_the_published_words_of_seed_1():
    """The words a prototype of the definition's text gave, kept as a pin on both definitions."""
    table = {1: (0xFC622C3E, 0x38464F30, 0x1D88BCE5), 64: (0xA5FD1558, 0xD9710906, 0x47C577C4)}
    for rounds, (i8, i8_injected, f16) in table.items():
        plain, injected = selftest_reference(1, rounds), selftest_reference(1, rounds, inject=True)
        assert (plain["mfma_i8"], injected["mfma_i8"], plain["mfma_f16"]) == (i8, i8_injected, f16)


@pytest.mark.parametrize("rounds", [1, 64])
@pytest.mark.parametrize("seed", SEEDS)
def test_inject_changes_mfma_i8_and_nothing_else(seed, rounds):
    plain, injected = selftest_reference(seed, rounds), selftest_reference(seed, rounds, inject=True)
    assert [u for u in SELFTEST_UNITS if plain[u] != injected[u]] == ["mfma_i8"]
    # one bit of one int8 element of row 0 of A: row 0 of the product moves, no other row
    a, _ = selftest_accumulators(seed, rounds)
    b, _ = selftest_accumulators(seed, rounds, inject=True)
    assert (a[0] != b[0]).any() and np.array_equal(a[1:], b[1:])


def test_the_words_depend_on_seed_rounds_and_position():
    a = selftest_reference(7, 2)
    for other in (selftest_reference(8, 2), selftest_reference(7, 3)):
        assert all(a[u] != other[u] for u in SELFTEST_UNITS)
    from amdvgpu.ops.calib import _selftest_fold
    ci, cf = selftest_accumulators(7, 2)
    assert _selftest_fold(ci) == a["mfma_i8"] and _selftest_fold(ci.T) != a["mfma_i8"]   # a transposed result shows
    assert _selftest_fold(cf) == a["mfma_f16"] and _selftest_fold(cf.T) != a["mfma_f16"]
    assert _selftest_fold(np.roll(ci, 1, axis=1)) != a["mfma_i8"]                          # and a mis-routed one


@pytest.mark.parametrize("seed", SEEDS)
def test_the_accumulators_stay_in_range_at_1024_rounds(seed):
    """In int64: the i8 accumulator never nears the instruction's overflow, every partial sum
    of the f16 test is an integer float32 holds exactly, and a float32 accumulation gives
    the integer result (selftest_accumulators asserts the last two step by step)."""
    ci, cf = selftest_accumulators(seed, 1024)
    assert ci.dtype == np.int64 and cf.dtype == np.int64
    assert np.abs(ci).max() < 1 << 29
    assert np.abs(cf).max() < 1 << 24
    assert np.abs(ci).max() > 1 << 16 and np.abs(cf).max() > 1 << 8   # and the test is not degenerate


def test_the_tool_prints_the_words_without_rocm():
    env = {"PATH": os.environ.get("PATH", "/usr/bin:/bin"), "LD_LIBRARY_PATH": ""}
    p = tool("--selftest-expected", "9", "3", env=env)
    assert p.returncode == 0
    assert {l.split()[0]: int(l.split()[1]) for l in p.stdout.splitlines()} == selftest_reference(9, 3)


def test_usage_errors_exit_2():
    assert tool("--selftest-expected").returncode == 2
    assert tool("--selftest-expected", "1").returncode == 2
    assert tool("--selftest-expected", "1", "0").returncode == 2          # rounds 1..1024
    assert tool("--selftest-expected", "1", "1025").returncode == 2
    assert tool("--selftest-expected", str(1 << 32), "1").returncode == 2  # seed is 32 bits
    assert tool("--selftest-expected", "1", "1", "poke").returncode == 2
    assert tool("--selftest-expected", "1", "1", "inject", "x").returncode == 2
    for bad in ((1 << 32, 1), (1, 0), (1, 1025)):
        with pytest.raises(ValueError):
            selftest_reference(*bad)
