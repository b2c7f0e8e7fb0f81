"""vgpu-validate --conformance on the CPU: the pattern definition (numpy against the tool's
host C++, which the gfx950 kernels share), and the whole tool against the fake ROCr + HIP
(native/tests/fake/, fake_hip_module.cpp) under the preloaded shim - the "container" is
built with apply_contract like the other vGPU tests'.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from amdvgpu.ops import pattern_reference
from amdvgpu.shim.launcher import apply_contract, vgpu_env
from amdvgpu.shim.native import LIB_DIR, VALIDATE, lib_path

GiB = 1 << 30
FAKE_DIR = os.path.join(LIB_DIR, "fakerocm")
UUID = "GPU-fa4e000000000000"


def tool(*args, env=None):
    return subprocess.run([lib_path(VALIDATE), *args], env=env, capture_output=True, text=True, timeout=120)


# ---------------------------------------------------------------- the pattern definition

@pytest.mark.parametrize("n,seed,base", [(1024, 0x1234ABCD, 0), (1024, 1, 0), (64, 0xFFFFFFFF, 2**32 - 8),
                                         (16, 77, 2**40 + 3)])
def test_pattern_reference_equals_the_host_definition(n, seed, base):
    p = tool("--pattern", str(n), str(seed), str(base))
    assert p.returncode == 0, p.stderr
    want = np.array([int(x) for x in p.stdout.split()], dtype=np.uint32)
    got = pattern_reference(n, seed, base)
    assert got.dtype == np.uint32 and got.shape == (n,)
    assert np.array_equal(got, want)


def test_pattern_depends_on_index_and_seed():
    a = pattern_reference(4096, 5)
    assert len(set(a.tolist())) > 4090                      # no stuck or short-period range
    assert (a != pattern_reference(4096, 6)).mean() > 0.99  # a stale fill fails
    assert (a != pattern_reference(4096, 5, base=4096)).mean() > 0.99
    assert np.array_equal(a[8:], pattern_reference(4088, 5, base=8))   # base is an offset
    assert np.array_equal(a[3:], pattern_reference(4093, 5, base=3))   # ... of any alignment
    with pytest.raises(ValueError):
        pattern_reference(4, 1 << 32)


def test_decode_and_pattern_need_no_rocm(tmp_path):
    """The tool links no GPU library and brings its own C++ runtime: with nothing but the
    system's default library directories it still decodes and prints the pattern."""
    env = {"PATH": os.environ.get("PATH", "/usr/bin:/bin"), "LD_LIBRARY_PATH": ""}
    f = tmp_path / "allow"
    f.write_text("GPU-ABCDEF0123456789\n")
    p = tool("--decode", str(f), env=env)
    assert p.returncode == 0 and p.stdout.split() == ["GPU-abcdef0123456789"]
    p = tool("--pattern", "4", "9", env=env)
    assert p.returncode == 0 and [int(x) for x in p.stdout.split()] == pattern_reference(4, 9).tolist()
    needed = subprocess.run(["readelf", "-d", lib_path(VALIDATE)], capture_output=True, text=True).stdout
    libs = [l.split("[")[1].rstrip("]") for l in needed.splitlines() if "(NEEDED)" in l]
    assert libs and all(l.startswith(("libc.so", "libdl.so", "libpthread.so", "libm.so", "ld-linux")) for l in libs), libs


def test_usage_errors_exit_2():
    assert tool("--conformance", "--bytes", "100").returncode == 2      # not a multiple of 16
    assert tool("--conformance", "--inject", "0").returncode == 2
    assert tool("--conformance", "--frobnicate").returncode == 2
    assert tool("--pattern", "4").returncode == 2


# ---------------------------------------------------------------- the tool on the fake runtime

@pytest.fixture
def container(tmp_path):
    """env(contract, gpus=...) -> the environment of a process in a vGPU container on a node
    with the fake runtime."""
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


def test_two_agents_with_different_quotas_pass(container):
    c = vgpu_env(per_device_mem=[2 * GiB, 3 * GiB], cu_limit=50, cu_mode="spatial", shared_cache=container.region)
    rep, p = conformance(container(c, gpus=2))
    assert rep["ok"], p.stdout
    assert [d["device"] for d in rep["devices"]] == [0, 1]
    for d, quota in zip(rep["devices"], (2 * GiB, 3 * GiB)):
        ch = d["checks"]
        assert set(statuses(d).values()) == {"pass"}, ch
        assert list(ch) == ["shim", "quota", "oom", "cus", "gate", "memory"]
        assert ch["quota"]["total"] == ch["quota"]["promised"] == ch["quota"]["region_limit"] == quota
        assert ch["cus"]["census"] == ch["cus"]["reported"] == ch["cus"]["promised"] == 128
        assert ch["cus"]["mode"] == "spatial"
        assert ch["gate"]["counted"] >= ch["gate"]["launched"] > 0
        assert ch["memory"]["mismatches"] == 0 and ch["memory"]["first_index"] is None
        assert d["uuid"].startswith("GPU-")
    # --device picks one; the text form has one line per check
    p = tool("--conformance", "--device", "1", "--bytes", "1m", env=container(c, gpus=2))
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and len(lines) == 6 and all(l.startswith("device 1 GPU-") for l in lines), p.stdout
    assert lines[1].split()[3:5] == ["quota", "pass"]
    assert tool("--conformance", "--device", "5", "--json", env=container(c, gpus=2)).returncode == 1


def test_a_smaller_promise_fails_quota_only(container, tmp_path):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_mode="spatial", shared_cache=container.region)
    limits = tmp_path / "limits"
    limits.write_text(f"VGPU_DEVICE_MEMORY_LIMIT_0=1024m\nVGPU_DEVICE_CU_LIMIT_0=50\nVGPU_CU_MODE=spatial\n"
                      f"VGPU_SHARED_CACHE={container.region}\n")
    rep, p = conformance(container(c), "--limits", str(limits))
    assert p.returncode == 1
    st = statuses(rep["devices"][0])
    assert st.pop("quota") == "fail" and set(st.values()) == {"pass"}, rep
    q = rep["devices"][0]["checks"]["quota"]
    assert q["promised"] == GiB and q["total"] == 2 * GiB


def test_a_wrong_cu_range_fails_cus_under_spatial(container, tmp_path):
    c = vgpu_env(mem_limit=2 * GiB, cu_limit=50, cu_range=(0, 128), cu_mode="spatial", shared_cache=container.region)
    limits = tmp_path / "limits"
    limits.write_text(f"VGPU_DEVICE_MEMORY_LIMIT_0=2048m\nVGPU_DEVICE_CU_RANGE_0=0-64\n"
                      f"VGPU_SHARED_CACHE={container.region}\n")
    rep, p = conformance(container(c), "--limits", str(limits))
    st = statuses(rep["devices"][0])
    assert p.returncode == 1 and st.pop("cus") == "fail" and set(st.values()) == {"pass"}, rep
    cus = rep["devices"][0]["checks"]["cus"]
    assert cus["census"] == cus["reported"] == 128 and cus["promised"] == 64
    # the same mismatch under the GPU-time limiter is reported, not failed: no mask is promised there
    c["VGPU_CU_MODE"] = "temporal"
    rep, p = conformance(container(c), "--limits", str(limits))
    cus = rep["devices"][0]["checks"]["cus"]
    assert p.returncode == 0 and cus["status"] == "info" and cus["mode"] == "temporal" and cus["census"] == 256, rep


def test_without_the_shim_everything_else_is_skipped(container):
    rep, p = conformance(container({}, shim=False))
    st = statuses(rep["devices"][0])
    assert p.returncode == 1 and st.pop("shim") == "fail" and set(st.values()) == {"skip"}, rep
    assert rep["devices"][0]["checks"]["shim"]["reason"]
    # a region path that nobody keeps is the same finding
    rep, p = conformance(container({}, shim=False, VGPU_SHARED_CACHE=container.region))
    assert p.returncode == 1 and statuses(rep["devices"][0])["shim"] == "fail"


def test_injected_words_are_all_found(container):
    c = vgpu_env(mem_limit=2 * GiB, shared_cache=container.region)
    rep, p = conformance(container(c), "--inject", "3")
    mem = rep["devices"][0]["checks"]["memory"]
    assert p.returncode == 1 and mem["status"] == "fail" and mem["mismatches"] == 3 and mem["injected"] == 3, rep
    assert mem["first_index"] == 0
    st = statuses(rep["devices"][0])
    assert [k for k, v in st.items() if v == "fail"] == ["memory"], st


def test_split_duplicates_are_two_devices_with_their_own_quota(container):
    c = vgpu_env(per_device_mem=[GiB, 2 * GiB], device_map=[UUID, UUID], shared_cache=container.region,
                 extra={"VGPU_DUPLICATE_SPLIT": "1"})
    rep, p = conformance(container(c))
    assert p.returncode == 0 and len(rep["devices"]) == 2, p.stdout + p.stderr[-1000:]
    for d, quota in zip(rep["devices"], (GiB, 2 * GiB)):
        q = d["checks"]["quota"]
        assert q["status"] == "pass" and q["total"] == q["promised"] == q["region_limit"] == quota, rep
        assert d["checks"]["oom"]["status"] == "pass" and d["checks"]["memory"]["status"] == "pass"
    assert rep["devices"][0]["uuid"] != rep["devices"][1]["uuid"]   # the second vGPU's own identity


def test_no_runtime_is_a_failed_check_not_a_crash(tmp_path):
    env = {"PATH": os.environ.get("PATH", "/usr/bin:/bin"), "LD_LIBRARY_PATH": str(tmp_path), "FAKE_ROCR_GPUS": "0"}
    p = tool("--conformance", "--json", env=env)
    rep = json.loads(p.stdout)
    assert p.returncode == 1 and rep["version"] == 1 and not rep["ok"]
    # no runtime, or a runtime without a GPU: a failed "runtime"; on a GPU node the default ROCm
    # directory still serves one, and what fails is "shim"
    if rep["devices"]:
        assert all(d["checks"]["shim"]["status"] == "fail" for d in rep["devices"])
    else:
        assert rep["runtime"]["status"] == "fail" and rep["runtime"]["reason"]
