"""The device identity of split duplicate vGPUs on a real MI355X (--duplicate-vgpus=split with
--virtual-pci-ids on): one GPU named twice (4 GiB and 6 GiB vGPUs), as in test_gpu_split.py.
The second vGPU reports a PCI bus id and UUID of its own, pointers and streams report the vGPU
they were made on - also from a thread on the other vGPU and for interior pointers - and a
stream-ordered allocation is charged to its stream's vGPU. First a stand-alone HIP program
(native/tests/vdev_probe.hip), then stock PyTorch.

No over-quota stream-ordered allocation here: the ROCm 7.x runtime crashes after a refused pool
chunk (hip_hooks.cpp), so that edge is covered on the fake runtime only (test_vdev_identity.py).
"""
import json
import os
import subprocess

import pytest

from amdvgpu.shim.launcher import popen, vgpu_env
from amdvgpu.shim.native import LIB_DIR
from amdvgpu.shim.region import Region
from conftest import run_child

pytestmark = pytest.mark.gpu
GiB = 1 << 30
MiB = 1 << 20
PROBE = os.path.join(LIB_DIR, "vdev_probe")


def _gpu():
    from amdvgpu.plugin.devices import SysfsBackend
    devs = SysfsBackend().devices()
    assert devs, "no GPU in sysfs"
    return devs[0]


def _contract(tmp_region, ids="1", **extra):
    g = _gpu()
    # the plugin's contract for two vGPUs of one GPU (contract.py), as in test_gpu_split.py
    return vgpu_env(shared_cache=tmp_region, device_map=[g.uuid, g.uuid], per_device_mem=[4 * GiB, 6 * GiB],
                    extra={"VGPU_DUPLICATE_SPLIT": "1", "VGPU_VIRTUAL_PCI_IDS": ids,
                           "ROCR_VISIBLE_DEVICES": f"{g.uuid},{g.uuid}", "HIP_VISIBLE_DEVICES": "0,1",
                           "VGPU_DEVICE_BDFS": f"{g.bdf},{g.bdf}", **extra})


def _parse(bus):
    dom, b, rest = bus.split(":")
    d, f = rest.split(".")
    return int(dom, 16), int(b, 16), int(d, 16), int(f, 16)


def _slot_usage(path):
    """Bytes charged to the quota slots of vGPU 0 and vGPU 1: with one GPU agent (slot 0, the
    summed quota) they are slots 1 and 2."""
    with Region(path) as r:
        return r.device(1)["used"], r.device(2)["used"]


def test_probe_two_threads_on_the_two_vgpus(tmp_region):
    p = popen([PROBE, "--handshake"], _contract(tmp_region), stdin=subprocess.PIPE, stdout=subprocess.PIPE,
              stderr=subprocess.PIPE, text=True)
    usage = {}
    try:
        for phase in ("before", "after"):
            line = p.stdout.readline()
            assert line and json.loads(line) == {"phase": phase}, (line, p.stderr.read()[-3000:] if not line else "")
            usage[phase] = _slot_usage(tmp_region)
            p.stdin.write("\n")
            p.stdin.flush()
        out, err = p.communicate(timeout=120)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    assert p.returncode == 0, err[-3000:]
    r = json.loads(out.strip().splitlines()[-1])
    print("vdev_probe:", r, "slot usage:", usage)
    d0, d1 = r["dev"]
    # ids: distinct, device 0 the GPU's own, device 1 in domain real + 0x1000
    g = _gpu()
    assert _parse(d0["bus"]) == _parse(g.bdf), (d0, g.bdf)
    dom, bus, dev, fn = _parse(d0["bus"])
    assert _parse(d1["bus"]) == (dom + 0x1000, bus, dev, fn), (d0, d1)
    assert d0["prop"] == [dom, bus, dev] and d1["prop"] == [dom + 0x1000, bus, dev], r
    u0, u1 = bytes.fromhex(d0["uuid"]), bytes.fromhex(d1["uuid"])
    assert u1[:1] == b"g" and u1[1:] == u0[1:] and u0[:1] != b"g", (u0, u1)
    assert (d0["by_bus"], d1["by_bus"]) == (0, 1) and (d0["current"], d1["current"]) == (0, 1), r
    # streams and pointers report their vGPU, to their own thread and to T0
    assert (d0["stream_dev"], d1["stream_dev"]) == (0, 1), r
    t0 = r["from_t0"]
    assert t0["stream1"] == 1 and t0["ptr1"] == [1, 1] and t0["aptr1"] == [1, 1] and t0["attrs1"] == 1, t0
    assert t0["ptr0"] == [0, 0] and t0["aptr0"] == [0, 0], t0
    # one kernel per device on its own stream: every word, the tail included
    assert r["words"] == 256 * 1024 + 3 and (d0["bad"], d1["bad"]) == (0, 0), r
    # T1's stream-ordered 256 MiB (between the two readings) was charged to its stream's vGPU
    grew = [usage["after"][i] - usage["before"][i] for i in (0, 1)]
    assert usage["before"][0] >= 64 * MiB and usage["before"][1] >= 64 * MiB, usage
    assert grew[1] >= 256 * MiB and grew[0] < 256 * MiB, usage


TORCH = """
import ctypes, threading
hip = ctypes.CDLL("libamdhip64.so")

def bus_id(d):
    buf = ctypes.create_string_buffer(64)
    rc = hip.hipDeviceGetPCIBusId(buf, 64, d)
    return [rc, buf.value.decode()]

def by_bus(s):
    d = ctypes.c_int(-1)
    rc = hip.hipDeviceGetByPCIBusId(ctypes.byref(d), s.encode())
    return [rc, d.value]

if os.environ.get("IDENTITY_ONLY") == "1":
    ids = [bus_id(d) for d in range(2)]
    emit(ids=ids, by_bus=[by_bus(s) for _rc, s in ids])
    sys.exit(0)

import torch
n = torch.cuda.device_count()
props = [torch.cuda.get_device_properties(d) for d in range(n)]
ids = [bus_id(d) for d in range(n)]
big = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:1")
small = torch.full((1 << 20,), 7, dtype=torch.uint8, device="cuda:1")
small2 = torch.empty(256 << 10, dtype=torch.uint8, device="cuda:1")
stream = torch.cuda.Stream(device=1)
torch.cuda.synchronize(1)
seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= small2.data_ptr() < s["address"] + s["total_size"]]

class Wrapped:
    # only the CUDA array interface: the consumer has to find the device from the pointer
    def __init__(self, t):
        self.__cuda_array_interface__ = {"shape": (t.numel(),), "typestr": "|u1", "data": (t.data_ptr(), False),
                                         "version": 2}

def ordinal(ptr):
    v = ctypes.c_int(-1)
    rc = hip.hipPointerGetAttribute(ctypes.byref(v), 9, ctypes.c_void_p(ptr))   # HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL
    return [rc, v.value]

out = {}
def on_device_0():
    torch.cuda.set_device(0)
    out["current"] = torch.cuda.current_device()
    out["ptrs"] = [ordinal(big.data_ptr()), ordinal(small.data_ptr()), ordinal(small.data_ptr() + 4096),
                   ordinal(small2.data_ptr())]
    d = ctypes.c_int(-1)
    rc = hip.hipStreamGetDevice(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(d))
    out["stream"] = [rc, d.value]
    try:
        t = torch.as_tensor(Wrapped(small))
        out["as_tensor"] = [str(t.device), int(t[:16].sum().item())]
        out["as_tensor_cuda"] = str(torch.as_tensor(Wrapped(small), device="cuda").device)
    except Exception as e:
        out["as_tensor_error"] = repr(e)
th = threading.Thread(target=on_device_0)
th.start()
th.join()
emit(n=n, ids=ids, by_bus=[by_bus(s) for _rc, s in ids],
     interior=bool(seg) and small2.data_ptr() > seg[0]["address"],
     prop_ids=[[p.pci_domain_id, p.pci_bus_id, p.pci_device_id] if hasattr(p, "pci_bus_id") else None for p in props],
     **out)
"""


def test_stock_pytorch_sees_each_vgpus_identity(tmp_region):
    res, p = run_child(TORCH, _contract(tmp_region), timeout=120, check=False)
    assert res, p.stderr[-3000:]
    r = res[0]
    print("torch child:", r)
    assert r["n"] == 2 and [rc for rc, _s in r["ids"]] == [0, 0], r
    a, b = (_parse(s) for _rc, s in r["ids"])
    assert a != b and b == (a[0] + 0x1000, a[1], a[2], a[3]), r
    assert r["by_bus"] == [[0, 0], [0, 1]], r
    if r["prop_ids"][0] is not None:   # this torch exposes the properties' PCI fields
        assert r["prop_ids"] == [list(a[:3]), list(b[:3])], r
    # from a thread whose current device is 0: the cuda:1 tensors (the second small one is an
    # interior pointer of a caching-allocator segment, small + 4096 of a block) and the stream
    assert r["current"] == 0 and r["interior"], r
    assert r["ptrs"] == [[0, 1]] * 4, r
    assert r["stream"] == [0, 1], r
    # PyTorch takes the device of a bare __cuda_array_interface__ object from its pointer
    assert "as_tensor_error" not in r, r
    assert r["as_tensor"] == ["cuda:1", 7 * 16], r
    # the control: without virtual ids both vGPUs report the GPU's own bus id
    res, p = run_child(TORCH, _contract(tmp_region + ".off", ids="0", IDENTITY_ONLY="1"), timeout=120, check=False)
    try:
        assert res, p.stderr[-3000:]
        ids = res[0]["ids"]
        assert ids[0] == ids[1] == [0, r["ids"][0][1]], res
    finally:
        if os.path.exists(tmp_region + ".off"):
            os.unlink(tmp_region + ".off")
