"""The compute known-answer kernel (cu_selftest in native/src/kernels/device_kernels.h,
amdvgpu.ops.cu_selftest) and vgpu-validate --conformance --compute on a real MI355X: integer
results, exact equality with the numpy definition (selftest_reference, which
tests/test_selftest_reference.py pins to the C definition).

One child process runs every shape once; the tests assert on what it reports. Shapes: 1 and 2
workgroups (one and two records of four waves), 300 (more workgroups than CUs), each with 1, 2
and 64 rounds (one pass of the loops, the first repeat, the tool's count).
"""
import json
import subprocess

import pytest

from amdvgpu.shim.launcher import apply_contract, vgpu_env
from amdvgpu.shim.native import VALIDATE, lib_path
from conftest import run_child

pytestmark = pytest.mark.gpu

GiB = 1 << 30
NBLOCKS = [1, 2, 300]
ROUNDS = [1, 2, 64]

CHILD = """
import ctypes
import numpy as np, torch
from amdvgpu.ops import cu_census, cu_selftest, selftest_reference
from amdvgpu.ops.calib import SELFTEST_UNITS, _k
GUARD, G = 64, 0xA5A5A5A5
P = ctypes.c_void_p
SEED = 0x5EED0001

def raw(nblocks, rounds):
    whole = torch.full((2 * GUARD + 32 * nblocks,), G - (1 << 32), dtype=torch.int32, device="cuda")
    rc = _k().vgpu_cu_selftest(P(whole.data_ptr() + 4 * GUARD), nblocks, SEED, rounds, 10, None, 0, None)
    torch.cuda.synchronize()
    h = whole.cpu().numpy().view(np.uint32)
    rec = h[GUARD:-GUARD].reshape(4 * nblocks, 8)
    want = selftest_reference(SEED, rounds)
    return dict(rc=rc, guards=bool((h[:GUARD] == G).all() and (h[-GUARD:] == G).all()),
                equal=bool((rec[:, 1:5] == np.array([want[u] for u in SELFTEST_UNITS], dtype=np.uint32)).all()),
                zeros=bool((rec[:, 5:] == 0).all()), loc_bits=bool((rec[:, 0] >> 18 == 0).all()))

shapes, injected = {}, {}
for nblocks in %r:
    for rounds in %r:
        key = "%%d-%%d" %% (nblocks, rounds)
        shapes[key] = raw(nblocks, rounds)
        r = cu_selftest(nblocks, rounds, seed=SEED, hold_us=10, inject=[0, nblocks - 1])
        injected[key] = dict(waves=r["waves"], bad=[[b["block"], b["wave"], b["units"]] for b in r["bad"]])

full = cu_census()
r = cu_selftest(300, 2, hold_us=10)
clean = dict(waves=r["waves"], bad=r["bad"], inside=bool(r["cus"] <= full), simd_pairs=r["simd_pairs"], cus=len(r["cus"]))

x = torch.zeros(32, dtype=torch.int32, device="cuda")
args = dict(null=_k().vgpu_cu_selftest(None, 1, 1, 1, 0, None, 0, None),
            rounds0=_k().vgpu_cu_selftest(P(x.data_ptr()), 1, 1, 0, 0, None, 0, None),
            rounds1025=_k().vgpu_cu_selftest(P(x.data_ptr()), 1, 1, 1025, 0, None, 0, None),
            bad65=_k().vgpu_cu_selftest(P(x.data_ptr()), 1, 1, 1, 0, P(x.data_ptr()), 65, None),
            bad_null=_k().vgpu_cu_selftest(P(x.data_ptr()), 1, 1, 1, 0, None, 1, None),
            blocks0=_k().vgpu_cu_selftest(P(x.data_ptr()), 0, 1, 1, 0, None, 0, None))
torch.cuda.synchronize()
emit(shapes=shapes, injected=injected, clean=clean, args=args, untouched=bool((x == 0).all()))
""" % (NBLOCKS, ROUNDS)

SLICE_CHILD = """
import torch
from amdvgpu.ops import cu_census, cu_selftest
census = cu_census(8192, 300)
r = cu_selftest()
emit(census=len(census), cus=len(r["cus"]), same=bool(r["cus"] == census), bad=r["bad"], waves=r["waves"],
     simd_pairs=r["simd_pairs"], reported=torch.cuda.get_device_properties(0).multi_processor_count)
"""


@pytest.fixture(scope="module")
def results():
    res, _ = run_child(CHILD, None, timeout=120)
    return res[0]


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("nblocks", NBLOCKS)
def test_every_wave_equals_the_reference(results, nblocks, rounds):
    r = results["shapes"]["%d-%d" % (nblocks, rounds)]
    assert r["rc"] == 0
    assert r["equal"], "a wave's word differs from selftest_reference"
    assert r["zeros"] and r["loc_bits"], "a record's spare words or its location are malformed"
    assert r["guards"], "a word outside the output was written"


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("nblocks", NBLOCKS)
def test_injection_turns_wave_0_of_the_listed_workgroups_wrong(results, nblocks, rounds):
    r = results["injected"]["%d-%d" % (nblocks, rounds)]
    assert r["waves"] == 4 * nblocks
    assert r["bad"] == [[b, 0, ["mfma_i8"]] for b in sorted({0, nblocks - 1})], r


def test_a_clean_run_reports_no_wave_and_real_cus(results):
    c = results["clean"]
    assert c["waves"] == 1200 and c["bad"] == []
    assert c["inside"] and 1 <= c["cus"] <= 256 and c["cus"] <= c["simd_pairs"] <= 4 * c["cus"]


def test_bad_arguments_are_refused(results):
    assert set(results["args"].values()) == {-1}, results["args"]
    assert results["untouched"]


def test_the_default_grid_covers_a_half_gpu_slice(tmp_region):
    c = vgpu_env(mem_limit=8 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=tmp_region)
    res, _ = run_child(SLICE_CHILD, c, timeout=120)
    r = res[0]
    print(r)
    assert r["bad"] == [] and r["waves"] == 8192
    assert r["cus"] == r["census"] == r["reported"] == 128 and r["same"]


def conformance(contract, *args):
    env = apply_contract(contract, preload=True)
    p = subprocess.run([lib_path(VALIDATE), "--conformance", "--json", "--bytes", "16MiB", *args], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode in (0, 1), (p.returncode, p.stderr[-2000:])
    rep = json.loads(p.stdout)
    assert rep["version"] == 1 and rep["ok"] == (p.returncode == 0), p.stdout
    print(p.stdout)
    return rep, p


def failed(dev):
    return sorted(k for k, v in dev["checks"].items() if v["status"] == "fail")


def test_the_tool_passes_compute_on_the_promised_vgpu(tmp_region):
    c = vgpu_env(mem_limit=8 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=tmp_region)
    rep, p = conformance(c, "--compute")
    assert p.returncode == 0 and failed(rep["devices"][0]) == [], p.stdout
    ch = rep["devices"][0]["checks"]
    assert list(ch) == ["shim", "quota", "oom", "cus", "gate", "memory", "compute"]
    comp = ch["compute"]
    assert comp["status"] == "pass" and comp["bad_waves"] == 0 and comp["waves"] == 8192 and comp["rounds"] == 64
    assert comp["cus"] == comp["reported"] == 128 and comp["mode"] == "spatial"
    assert comp["cus"] <= comp["simd_pairs"] <= 4 * comp["cus"]


def test_the_tool_finds_injected_workgroups(tmp_region):
    c = vgpu_env(mem_limit=8 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=tmp_region)
    rep, p = conformance(c, "--compute", "--inject-compute", "5")
    assert p.returncode == 1 and failed(rep["devices"][0]) == ["compute"], rep
    comp = rep["devices"][0]["checks"]["compute"]
    assert comp["bad_waves"] == 5 and comp["injected"] == 5
    assert len(comp["bad"]) == 5 and all(b["units"] == ["mfma_i8"] for b in comp["bad"]), comp
