"""--virtual-pci-ids (env VIRTUAL_PCI_IDS, default on): the contract of a container holding two
vGPUs of one GPU carries VGPU_VIRTUAL_PCI_IDS=1|0 together with VGPU_DUPLICATE_SPLIT=1, and
never without it (tests/test_vdev_identity.py runs the shim side)."""
import grpc
import pytest

from amdvgpu.plugin.config import parse_config
from amdvgpu.plugin.devices import FakeBackend
from test_plugin_grpc import plugin_dir, shutdown, start  # noqa: F401  (fixture)


def _allocate_two_of_one_gpu(plugin_dir, **kw):  # noqa: F811
    cfg, k, sup, stop, th = start(plugin_dir, device_split_count=4, backend=FakeBackend(n=1), **kw)
    try:
        k.wait_registered("amd.com/gpu")
        k.wait_devices("amd.com/gpu", predicate=lambda d: len(d) == 4)
        _ids, resp = k.allocate("amd.com/gpu", 2)
        return cfg, dict(resp.envs)
    finally:
        shutdown(k, stop, th)


def test_default_allocate_of_two_vgpus_of_one_gpu_carries_virtual_ids(plugin_dir):  # noqa: F811
    cfg, envs = _allocate_two_of_one_gpu(plugin_dir)
    assert cfg.virtual_pci_ids == "on" and cfg.duplicate_vgpus == "split"
    assert envs["VGPU_DUPLICATE_SPLIT"] == "1" and envs["VGPU_VIRTUAL_PCI_IDS"] == "1", envs


def test_virtual_pci_ids_off(plugin_dir):  # noqa: F811
    _cfg, envs = _allocate_two_of_one_gpu(plugin_dir, virtual_pci_ids="off")
    assert envs["VGPU_DUPLICATE_SPLIT"] == "1" and envs["VGPU_VIRTUAL_PCI_IDS"] == "0", envs


def test_merge_carries_neither(plugin_dir):  # noqa: F811
    _cfg, envs = _allocate_two_of_one_gpu(plugin_dir, duplicate_vgpus="merge")
    assert "VGPU_VIRTUAL_PCI_IDS" not in envs and "VGPU_DUPLICATE_SPLIT" not in envs, envs


def test_reject_carries_neither(plugin_dir):  # noqa: F811
    with pytest.raises(grpc.RpcError) as e:
        _allocate_two_of_one_gpu(plugin_dir, duplicate_vgpus="reject")
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT


def test_one_vgpu_carries_neither(plugin_dir):  # noqa: F811
    cfg, k, sup, stop, th = start(plugin_dir, device_split_count=4, backend=FakeBackend(n=1))
    try:
        k.wait_registered("amd.com/gpu")
        k.wait_devices("amd.com/gpu", predicate=lambda d: len(d) == 4)
        _ids, resp = k.allocate("amd.com/gpu", 1)
        assert "VGPU_VIRTUAL_PCI_IDS" not in dict(resp.envs) and "VGPU_DUPLICATE_SPLIT" not in dict(resp.envs)
    finally:
        shutdown(k, stop, th)


def test_flag_env_and_validation():
    assert parse_config([], environ={}).virtual_pci_ids == "on"
    assert parse_config(["--virtual-pci-ids", "off"], environ={}).virtual_pci_ids == "off"
    assert parse_config([], environ={"VIRTUAL_PCI_IDS": "off"}).virtual_pci_ids == "off"
    assert parse_config(["--virtual-pci-ids", "on"], environ={"VIRTUAL_PCI_IDS": "off"}).virtual_pci_ids == "on"
    with pytest.raises(ValueError):
        parse_config(["--virtual-pci-ids", "maybe"], environ={})
