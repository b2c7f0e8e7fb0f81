"""vgpu-validate --conformance --compute on the CPU: the tool against the fake ROCr + HIP
(native/tests/fake/fake_hip_module.cpp emulates cu_selftest from vgpu/selftest.h) under the
preloaded shim, in a "container" built like those of tests/test_validate_conformance.py.
"""
import json
import os
import subprocess

import pytest

from amdvgpu.shim.launcher import apply_contract, vgpu_env
from amdvgpu.shim.native import LIB_DIR, VALIDATE, lib_path

GiB = 1 << 30
FAKE_DIR = os.path.join(LIB_DIR, "fakerocm")
OLD_CHECKS = ["shim", "quota", "oom", "cus", "gate", "memory"]
FIELDS = {"status", "waves", "cus", "reported", "simd_pairs", "rounds", "bad_waves", "mode", "ms"}


def tool(*args, env=None):
    return subprocess.run([lib_path(VALIDATE), *args], env=env, capture_output=True, text=True, timeout=120)


@pytest.fixture
def container(tmp_path):
    kfd = tmp_path / "kfd"
    kfd.mkdir()

    def env(contract, gpus=1, shim=True, **extra):
        base = {k: v for k, v in os.environ.items() if not k.startswith(("VGPU_", "FAKE_"))}
        base.update(FAKE_ROCR_GPUS=str(gpus), FAKE_ROCR_HBM=str(16 * GiB), FAKE_KFD_ROOT=str(kfd),
                    VGPU_KFD_ROOT=str(kfd), VGPU_LOCK_FILE=str(tmp_path / "lock" / "hostpid.lock"),
                    LD_LIBRARY_PATH=FAKE_DIR)
        base.update(extra)
        return apply_contract(contract if shim else {}, base_env=base, preload=shim)

    env.region = str(tmp_path / "region.cache")
    return env


def conformance(env, *args):
    p = tool("--conformance", "--json", "--bytes", "1m", *args, env=env)
    assert p.returncode in (0, 1), p.stderr[-2000:]
    rep = json.loads(p.stdout)
    assert rep["version"] == 1 and rep["ok"] == (p.returncode == 0)
    return rep, p


def statuses(dev):
    return {k: v["status"] for k, v in dev["checks"].items()}


def test_compute_passes_on_a_half_gpu_slice(container):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=container.region)
    rep, p = conformance(container(c), "--compute")
    assert p.returncode == 0 and rep["ok"], p.stdout
    ch = rep["devices"][0]["checks"]
    assert list(ch) == OLD_CHECKS + ["compute"]
    assert set(statuses(rep["devices"][0]).values()) == {"pass"}, ch
    comp = ch["compute"]
    assert set(comp) == FIELDS, comp
    assert comp["cus"] == comp["reported"] == 128 and comp["mode"] == "spatial"
    assert comp["waves"] == 8192 and comp["rounds"] == 64 and comp["bad_waves"] == 0
    assert comp["simd_pairs"] == 4 * 128
    # with --spill the check stands between memory and spill; the text form gains one line
    rep, p = conformance(container(c), "--compute", "--spill")
    assert list(rep["devices"][0]["checks"]) == OLD_CHECKS + ["compute", "spill"]
    p = tool("--conformance", "--compute", "--bytes", "1m", env=container(c))
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and len(lines) == 7 and lines[6].split()[3:5] == ["compute", "pass"], p.stdout


def test_without_the_flag_nothing_changes(container):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=container.region)
    rep, p = conformance(container(c))
    assert p.returncode == 0 and list(rep["devices"][0]["checks"]) == OLD_CHECKS


def test_injected_workgroups_are_all_found(container):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=container.region)
    rep, p = conformance(container(c), "--compute", "--inject-compute", "3")
    st = statuses(rep["devices"][0])
    assert p.returncode == 1 and [k for k, v in st.items() if v == "fail"] == ["compute"], st
    assert all(v == "pass" for k, v in st.items() if k != "compute"), st
    comp = rep["devices"][0]["checks"]["compute"]
    assert comp["bad_waves"] == 3 and comp["injected"] == 3 and comp["waves"] == 8192
    assert len(comp["bad"]) == 3 and all(b["units"] == ["mfma_i8"] for b in comp["bad"]), comp
    assert 1 <= comp["bad_cus"] <= 3 and comp["cus"] == comp["reported"] == 128
    # the most that can be asked for: 64 wrong waves counted, 16 of them listed
    rep, p = conformance(container(c), "--compute", "--inject-compute", "64")
    comp = rep["devices"][0]["checks"]["compute"]
    assert p.returncode == 1 and comp["bad_waves"] == comp["injected"] == 64 and len(comp["bad"]) == 16, comp


@pytest.mark.parametrize("unit", ["valu", "lds", "mfma_i8", "mfma_f16"])
def test_a_cu_that_computes_wrong_is_named_with_its_unit(container, unit):
    """Under the GPU-time limiter the queue may use all 256 CUs of the fake GPU, 2048 workgroups
    put 8 on each: the 32 waves on XCC 1 / SE 2 / CU 3 return a wrong word for one unit."""
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="temporal", shared_cache=container.region)
    rep, p = conformance(container(c, FAKE_HIP_SELFTEST_BAD=f"0x1203:{unit}"), "--compute")
    st = statuses(rep["devices"][0])
    assert p.returncode == 1 and [k for k, v in st.items() if v == "fail"] == ["compute"], st
    comp = rep["devices"][0]["checks"]["compute"]
    assert comp["bad_waves"] == 32 and comp["bad_cus"] == 1 and "injected" not in comp, comp
    assert len(comp["bad"]) == 16
    assert {b["location"].rsplit("/", 1)[0] for b in comp["bad"]} == {"1/2/0/3"}
    assert {b["location"].rsplit("/", 1)[1] for b in comp["bad"]} == {"0", "1", "2", "3"}
    assert all(b["units"] == [unit] for b in comp["bad"]), comp


def test_temporal_mode_passes_with_coverage_as_information(container):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="temporal", shared_cache=container.region)
    rep, p = conformance(container(c), "--compute")
    comp = rep["devices"][0]["checks"]["compute"]
    assert p.returncode == 0 and comp["status"] == "pass" and comp["mode"] == "temporal", rep
    assert comp["cus"] == 256 and comp["bad_waves"] == 0 and "bad" not in comp


def test_without_the_shim_compute_is_skipped(container):
    rep, p = conformance(container({}, shim=False), "--compute")
    st = statuses(rep["devices"][0])
    assert p.returncode == 1 and st.pop("shim") == "fail" and set(st.values()) == {"skip"}, rep
    assert list(rep["devices"][0]["checks"]) == OLD_CHECKS + ["compute"]
    assert rep["devices"][0]["checks"]["compute"]["reason"]


def test_usage_errors_exit_2():
    assert tool("--conformance", "--inject-compute", "3").returncode == 2       # only with --compute
    assert tool("--conformance", "--compute", "--inject-compute", "0").returncode == 2
    assert tool("--conformance", "--compute", "--inject-compute", "65").returncode == 2
    assert tool("--conformance", "--compute", "--inject-compute").returncode == 2
