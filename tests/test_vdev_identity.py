"""The device identity of split duplicate vGPUs (--duplicate-vgpus=split with --virtual-pci-ids on,
VGPU_VIRTUAL_PCI_IDS=1) on the CPU-only fake runtime: the second and later vGPUs of a GPU have a
PCI bus id and UUID of their own, pointers and streams report the vGPU they were made on, and a
stream-ordered allocation is admitted against and charged to its stream's vGPU.

One fake GPU, VGPU_DEVICE_MAP naming it twice (1 GiB and 2 GiB vGPUs) as in
test_duplicate_split.py; the driver is native/tests/fake/vdev_harness (host threads T0, T1, ...:
a step prefixed "t1:" runs on T1, which keeps its own current device).

Reference: duplicate vGPUs get virtual PCI bus ids (assigning_virtual_pcibusID
[device.c:81-117], [device.c:187-209]).
"""
import json
import os
import subprocess

from amdvgpu.shim.native import LIB_DIR
from test_shim_fake import fake  # noqa: F401  (fixture)

GiB = 1 << 30
MiB = 1 << 20
UUID = "GPU-fa4e000000000000"
UUID_B = "GPU-fa4e000000000001"
PHYS = "0000:05:00.0"            # the fake GPU 0's bus id; GPU 1 sits at 0000:15:00.0
VDEV_HARNESS = os.path.join(LIB_DIR, "fakerocm", "vdev_harness")


def run(env, *ops, timeout=60):
    p = subprocess.run([VDEV_HARNESS, *ops], env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def _env(fake, split=True, ids="1", **extra):  # noqa: F811
    return fake(gpus=1, VGPU_DEVICE_MAP=f"0:{UUID} 1:{UUID}", VGPU_DEVICE_MEMORY_LIMIT_0="1g",
                VGPU_DEVICE_MEMORY_LIMIT_1="2g", VGPU_DUPLICATE_SPLIT="1" if split else "0",
                VGPU_VIRTUAL_PCI_IDS=ids, **extra)


def _one(out, key):
    return [o for o in out if key in o]


def _parse(bus):
    dom, b, rest = bus.split(":")
    d, f = rest.split(".")
    return int(dom, 16), int(b, 16), int(d, 16), int(f, 16)


def _used(info):
    """Bytes charged to a vGPU's quota slot, from its own hipMemGetInfo."""
    return info["total"] - info["free"]


def test_bus_ids_and_uuids(fake):  # noqa: F811
    out = run(_env(fake), "ids=0", "ids=1", f"bybus={PHYS}", "bybus=1000:05:00.0", "bybus=1000:5:0.0",
              "bybus=05:00.0", "bybus=2000:05:00.0", "shortbus=1,12", "shortbus=1,13", "shortbus=0,12", "ids=2")
    a, b, none = _one(out, "ids")
    assert a["rc"] == [0] * 6 and b["rc"] == [0] * 6, out
    assert a["bus"] == PHYS and b["bus"] != a["bus"], out
    assert _parse(b["bus"]) == (0x1000, 0x05, 0, 0), b
    # the properties and the attributes agree with the strings
    for d in (a, b):
        dom, bus, dev, _fn = _parse(d["bus"])
        assert d["prop"] == [dom, bus, dev] and d["attr"] == [dom, bus, dev], d
        assert d["prop_uuid"] == d["uuid"], d
    ua, ub = bytes.fromhex(a["uuid"]), bytes.fromhex(b["uuid"])
    assert ua == UUID[4:].encode() and ub[1:] == ua[1:] and ub[:1] == b"g", (ua, ub)
    by = _one(out, "bybus")
    assert [(o["bybus"], o["rc"]) for o in by[:4]] == [(0, 0), (1, 0), (1, 0), (0, 0)], by
    assert by[4]["rc"] != 0, by                      # no third vGPU
    # a short buffer: as the runtime answers it (12 characters and the terminator)
    assert [o["shortbus"] != 0 for o in _one(out, "shortbus")] == [True, False, True], out
    assert none["rc"][0] != 0 and none["rc"][1] != 0, none   # no device 2


def test_three_vgpus_of_one_gpu_and_one_of_another(fake):  # noqa: F811
    e = fake(gpus=2, VGPU_DEVICE_MAP=f"0:{UUID} 1:{UUID} 2:{UUID} 3:{UUID_B}", VGPU_DUPLICATE_SPLIT="1",
             VGPU_VIRTUAL_PCI_IDS="1", **{f"VGPU_DEVICE_MEMORY_LIMIT_{i}": "1g" for i in range(4)})
    out = run(e, "count", *[f"ids={d}" for d in range(4)], "bybus=2000:05:00.0", "bybus=0000:15:00.0")
    assert _one(out, "count")[0]["count"] == 4
    ids = _one(out, "ids")
    assert len({d["bus"] for d in ids}) == 4 and len({d["uuid"] for d in ids}) == 4, ids
    assert [_parse(d["bus"])[0] for d in ids] == [0, 0x1000, 0x2000, 0], ids
    assert [bytes.fromhex(d["uuid"])[:1] for d in ids[:3]] == [b"f", b"g", b"h"], ids
    assert ids[3]["bus"] == "0000:15:00.0" and bytes.fromhex(ids[3]["uuid"]) == UUID_B[4:].encode(), ids   # GPU B: untouched
    assert [o["bybus"] for o in _one(out, "bybus")] == [2, 3], out


def test_opt_out_and_merge_keep_the_physical_identity(fake):  # noqa: F811
    out = run(_env(fake, ids="0"), "ids=0", "ids=1", f"bybus={PHYS}", "t1:dev=1", "t1:malloc=64m", "ptrdev=0,0",
              "t1:stream=create", "streamdev=0")
    a, b = _one(out, "ids")
    assert a["bus"] == b["bus"] == PHYS and a["uuid"] == b["uuid"] and a["prop"] == b["prop"] and a["attr"] == b["attr"], out
    assert _one(out, "bybus")[0] == {"bybus": 0, "rc": 0}
    assert _one(out, "ptrdev")[0]["ptrdev"] == [0, 0, 0], out      # the physical ordinal, as before
    assert _one(out, "streamdev")[0]["streamdev"] == 0, out        # the asking thread's view, as before
    out = run(_env(fake, split=False), "count", "ids=0", "ids=1")
    assert _one(out, "count")[0]["count"] == 1
    a, none = _one(out, "ids")
    assert a["bus"] == PHYS and bytes.fromhex(a["uuid"]) == UUID[4:].encode() and none["rc"][0] != 0, out


def test_pointers_report_the_vgpu_they_were_allocated_on(fake):  # noqa: F811
    out = run(_env(fake, FAKE_ROCR_REUSE="1"), "dev=0", "t1:dev=1", "t1:malloc=64m", "ptrdev=0,0", "ptrdev=0,1",
              f"ptrdev=0,{64 * MiB - 1}", "malloc=64m", "ptrdev=1,0", "t1:ptrdev=1,4096", "t1:free=0", "malloc=64m",
              "ptrdev=2,0", f"t1:ptrdev=2,{32 * MiB}")
    m = _one(out, "malloc")
    assert [o["malloc"] for o in m] == ["ok"] * 3 and m[2]["addr"] == m[0]["addr"] != m[1]["addr"], m
    p = _one(out, "ptrdev")
    assert all(o["rc"] == [0, 0, 0] for o in p), p
    assert [o["ptrdev"] for o in p[:3]] == [[1, 1, 1]] * 3, p        # T1's buffer, asked from T0: base and interior
    assert [o["ptrdev"] for o in p[3:5]] == [[0, 0, 0]] * 2, p       # T0's buffer, asked from T0 and from T1
    assert [o["ptrdev"] for o in p[5:]] == [[0, 0, 0]] * 2, p        # the freed address, allocated again on device 0


def test_streams_report_the_vgpu_they_were_created_on(fake):  # noqa: F811
    out = run(_env(fake), "dev=0", "t1:dev=1", "t1:stream=create", "t1:stream=flags", "t1:stream=priority",
              "t1:stream=cumask", *[f"streamdev={i}" for i in range(4)], "streamdev=-1", "t1:streamdev=-1",
              "t1:sdestroy=0", "stream=create", "streamdev=4", "t1:streamdev=4")
    assert all(o["rc"] == 0 for o in _one(out, "stream") + _one(out, "streamdev")), out
    got = [o["streamdev"] for o in _one(out, "streamdev")]
    assert got[:4] == [1, 1, 1, 1], got         # T1's streams, asked from T0
    assert got[4:6] == [0, 1], got              # the null stream: the asking thread's vGPU
    assert got[6:] == [0, 0], got               # after the destroy, a new stream on device 0


def test_stream_ordered_allocations_are_charged_to_the_streams_vgpu(fake):  # noqa: F811
    out = run(_env(fake), "dev=0", "t1:dev=1", "stream=create", "t1:stream=create", "t1:meminfo", "meminfo",
              "amalloc=1500m,1", "t1:meminfo", "meminfo", "ptrdev=0,0", f"ptrdev=0,{1500 * MiB - 1}",
              "t1:amalloc=1500m,0", "t1:pmalloc=1500m,0", "afree=0,1", "t1:meminfo", "meminfo",
              "t1:amalloc=900m,0", "t1:ptrdev=3,1", "t1:meminfo", "meminfo", "t1:afree=3,0", "meminfo")
    a = _one(out, "amalloc") + _one(out, "pmalloc")
    info = _one(out, "total")
    assert [o["total"] for o in info[:2]] == [2 * GiB, GiB], info
    assert (_used(info[0]), _used(info[1])) == (0, 0), info
    # T0 (device 0, 1 GiB) on T1's stream: admitted against and charged to vGPU 1 (2 GiB)
    assert a[0]["amalloc"] == "ok", a
    assert (_used(info[2]), _used(info[3])) == (1500 * MiB, 0), info
    assert [o["ptrdev"] for o in _one(out, "ptrdev")[:2]] == [[1, 1, 1]] * 2, out
    # T1 (device 1) on a device-0 stream: 1500 MiB is past vGPU 0's 1 GiB
    assert a[1]["amalloc"] == "oom" and a[3]["pmalloc"] == "oom", a
    # hipFreeAsync returns the charge
    assert (_used(info[4]), _used(info[5])) == (0, 0), info
    assert a[2]["amalloc"] == "ok" and _one(out, "ptrdev")[2]["ptrdev"] == [0, 0, 0], out
    assert (_used(info[6]), _used(info[7])) == (0, 900 * MiB), info
    assert _used(info[8]) == 0, info


def test_rccl_keeps_seeing_the_physical_gpu(fake):  # noqa: F811
    out = run(_env(fake), "rccl=1", "ids=1", "rccl=0")
    r1, r0 = _one(out, "rccl")
    direct = _one(out, "ids")[0]
    assert r1["rccl"] == 0 and r1["bus"] == PHYS and r1["uuid0"] == ord("f") and r1["domain"] == 0, r1
    assert direct["bus"] == "1000:05:00.0" and bytes.fromhex(direct["uuid"])[:1] == b"g", direct
    assert r0["rccl"] == 0 and r0["bus"] == PHYS and r0["bybus"] == 0, r0


def test_other_ordinals_are_mapped(fake):  # noqa: F811
    out = run(_env(fake), "dev=1", "ctxdev", "advise=1", "prefetch=1", "advise=2", "prefetch=2", "advise=0",
              "p2p=0,1", "p2p=1,0", "p2p=1,1", "p2p=0,2")
    assert _one(out, "ctxdev")[0] == {"ctxdev": 1, "rc": 0}
    adv = _one(out, "advise") + _one(out, "prefetch")
    ok = [o for o in adv if o.get("advise", o.get("prefetch")) == 0]
    assert len(ok) == 3 and all(o["runtime_id"] == 0 for o in ok), adv      # the runtime got physical device 0
    bad = [o for o in adv if o not in ok]
    assert len(bad) == 2 and all(o.get("advise", o.get("prefetch")) == 101 for o in bad), adv   # hipErrorInvalidDevice
    p = _one(out, "p2p")
    assert p[0]["rc"] == [0, 0, 0] and p[0]["p2p"][:2] == [1, 1] and p[0]["p2p"][2] >= 0, p
    assert p[1]["rc"] == [0, 0, 0] and p[1]["p2p"][:2] == [1, 1], p
    assert p[2]["rc"] == [101] * 3 and p[3]["rc"] == [101] * 3, p


def test_more_vgpus_than_quota_slots(fake):  # noqa: F811
    """2 GPUs x 8 vGPUs want 2 + 16 region slots of 16: the last two vGPUs have no quota of their
    own (their GPU's summed quota guards), and no slot index past the region's reaches it (the
    region's charge / limit / usage assert their bounds; vgpu_core_tests virtual_slots)."""
    dmap = " ".join(f"{i}:{UUID if i < 8 else UUID_B}" for i in range(16))
    e = fake(gpus=2, hbm=16 * GiB, VGPU_DEVICE_MAP=dmap, VGPU_DUPLICATE_SPLIT="1", VGPU_VIRTUAL_PCI_IDS="1",
             **{f"VGPU_DEVICE_MEMORY_LIMIT_{i}": f"{256 + 64 * i}m" for i in range(16)})
    ops = ["count"]
    for d in range(16):
        ops += [f"dev={d}", "meminfo", "malloc=100m", f"ptrdev={d},4096", "meminfo"]
    out = run(e, *ops, "ids=15", "bybus=7000:15:00.0")
    assert _one(out, "count")[0]["count"] == 16
    info = _one(out, "total")
    guard = sum(256 + 64 * i for i in range(8, 16)) * MiB            # GPU B's summed quota
    want = [(256 + 64 * d) * MiB for d in range(14)] + [guard, guard]
    assert [o["total"] for o in info[0::2]] == want, info
    assert [_used(o) for o in info[1::2]][:14] == [100 * MiB] * 14, info
    assert [o["malloc"] for o in _one(out, "malloc")] == ["ok"] * 16
    assert [o["ptrdev"] for o in _one(out, "ptrdev")] == [[d] * 3 for d in range(16)], out
    assert _parse(_one(out, "ids")[0]["bus"]) == (0x7000, 0x15, 0, 0) and _one(out, "bybus")[0]["bybus"] == 15, out


def test_pointer_queries_stay_suspend_gated(fake):  # noqa: F811
    """The three pointer entry points became hand-written hooks: each still blocks while the
    container is suspended and proceeds on resume (the 40 ms scheme of shim_harness' gates=)."""
    out = run(_env(fake), "t1:dev=1", "t1:malloc=1m", "ptrgates=0")
    res = _one(out, "ptrgates")[0]
    assert res["ptrgates"] == 3 and res["unrouted"] == [] and res["ungated"] == [] and res["unreached"] == [], res
    out = run(_env(fake, split=False), "malloc=1m", "ptrgates=0", "ptrdev=0,0")
    res = _one(out, "ptrgates")[0]
    assert res["unrouted"] == [] and res["ungated"] == [] and res["unreached"] == [], res
    assert _one(out, "ptrdev")[0]["ptrdev"] == [0, 0, 0]
