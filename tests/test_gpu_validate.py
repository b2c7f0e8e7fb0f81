"""vgpu-validate --conformance on a real MI355X: the tool, started like a process of a vGPU
container (apply_contract: the contract's environment and the preloaded shim), checks the
limits it was promised with its own embedded gfx950 kernels.
"""
import json
import subprocess

import pytest

from amdvgpu.shim.launcher import apply_contract, vgpu_env
from amdvgpu.shim.native import VALIDATE, lib_path

pytestmark = pytest.mark.gpu

GiB = 1 << 30
MiB = 1 << 20


def conformance(contract, *args):
    env = apply_contract(contract or {}, preload=contract is not None)
    if contract is None:
        for k in [k for k in env if k.startswith("VGPU_")]:
            del env[k]
    p = subprocess.run([lib_path(VALIDATE), "--conformance", "--json", *args], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode in (0, 1), (p.returncode, p.stderr[-2000:])
    rep = json.loads(p.stdout)
    assert rep["version"] == 1 and rep["ok"] == (p.returncode == 0), p.stdout
    print(p.stdout)
    return rep, p


def failed(dev):
    return sorted(k for k, v in dev["checks"].items() if v["status"] == "fail")


def test_the_promised_vgpu_passes(tmp_region):
    c = vgpu_env(mem_limit=8 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=tmp_region)
    rep, p = conformance(c, "--bytes", str(64 * MiB))
    assert p.returncode == 0, p.stdout
    ch = rep["devices"][0]["checks"]
    assert failed(rep["devices"][0]) == []
    assert ch["shim"]["status"] == "pass"
    assert ch["quota"]["status"] == "pass" and ch["quota"]["total"] == 8 * GiB
    assert ch["oom"]["status"] == "pass"
    assert ch["cus"]["status"] == "pass" and ch["cus"]["census"] == ch["cus"]["reported"] == 128
    assert ch["gate"]["status"] == "pass" and ch["gate"]["counted"] >= ch["gate"]["launched"] > 0
    assert ch["memory"]["status"] == "pass" and ch["memory"]["mismatches"] == 0


def test_a_wrong_promise_fails_quota_and_cus(tmp_region, tmp_path):
    c = vgpu_env(mem_limit=8 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=tmp_region)
    limits = tmp_path / "limits"
    limits.write_text(f"VGPU_DEVICE_MEMORY_LIMIT_0=4096m\nVGPU_DEVICE_CU_RANGE_0=0-64\nVGPU_CU_MODE=spatial\n"
                      f"VGPU_SHARED_CACHE={tmp_region}\n")
    rep, p = conformance(c, "--limits", str(limits), "--bytes", str(16 * MiB))
    assert p.returncode == 1
    assert failed(rep["devices"][0]) == ["cus", "quota"], rep
    assert rep["devices"][0]["checks"]["quota"]["promised"] == 4 * GiB
    assert rep["devices"][0]["checks"]["cus"]["promised"] == 64


def test_without_a_shim_the_check_fails_cleanly():
    rep, p = conformance(None, "--bytes", str(16 * MiB))
    assert p.returncode == 1 and rep["devices"], p.stdout
    for d in rep["devices"]:
        st = {k: v["status"] for k, v in d["checks"].items()}
        assert st.pop("shim") == "fail" and set(st.values()) == {"skip"}, d


def test_injected_words_fail_the_memory_check(tmp_region):
    c = vgpu_env(mem_limit=8 * GiB, shared_cache=tmp_region)
    rep, p = conformance(c, "--inject", "5", "--bytes", str(16 * MiB))
    mem = rep["devices"][0]["checks"]["memory"]
    assert p.returncode == 1 and failed(rep["devices"][0]) == ["memory"], rep
    assert mem["mismatches"] == 5 and mem["first_index"] == 0


def test_spilled_buffer_keeps_the_pattern(tmp_region):
    """Virtual device memory: 2 GiB HBM share of a 4 GiB quota. The buffer holds the pattern
    in host memory and after its promotion into HBM; when it never spills or is not promoted
    within the bound the tool says why (skip), and a mismatch is the only failure."""
    c = vgpu_env(mem_limit=4 * GiB, shared_cache=tmp_region, oversubscribe=True,
                 extra={"VGPU_DEVICE_HBM_LIMIT_0": "2048m"})
    rep, p = conformance(c, "--spill", "--bytes", "268435456")
    sp = rep["devices"][0]["checks"]["spill"]
    assert sp["status"] in ("pass", "skip"), rep
    assert sp.get("mismatches_spilled", 0) == 0 and sp.get("mismatches_promoted", 0) == 0
    if sp["status"] == "skip":
        assert sp["reason"]
    assert failed(rep["devices"][0]) == [] and p.returncode == 0, rep
