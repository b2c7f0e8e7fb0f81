#!/usr/bin/env python3
"""What a memory-heavy neighbour does to a pod's loads, level by level: a victim pod measures
pointer-chase latency (amdvgpu.ops.mem_latency: one lane per wave, one wave per CU of its
slice) over 1 MiB, 64 MiB and 2 GiB rings, alone and next to 1, 2 and 3 aggressor pods that run
back-to-back 100 ms mem_stream kernels over a 2 GiB buffer each, reading or writing.

The pods are split-4 vGPUs of one GPU from a real Allocate (NodeHarness), by default with
--cu-mode spatial, so every pod has CUs of its own: what is left to share is L2, Infinity
Cache, fabric and HBM. The four pod processes live for the whole run (at most 4 GPU
processes, each under its own `timeout`); the arms alternate (alone, read x1..x3, write x1..x3,
and again), and the script stops at the first child that exits.

The 1 MiB and 64 MiB rings are measured after an identical untimed launch. The 2 GiB ring is
measured cold: every launch takes a fresh chain_base, so it walks lines that no earlier launch
of this run has touched (one 64th of the ring per launch, 63 launches in a default run).

    python3 benchmarks/mem_interference.py --repeats 3 --json-out out.json --md-out out.md
"""
import argparse
import json
import os
import queue
import statistics
import subprocess
import sys
import tempfile
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {"1 MiB": 1 << 20, "64 MiB": 64 << 20, "2 GiB": 2 << 30}
COLD = 256 << 20              # rings above the Infinity Cache are measured without a warm launch
STREAM_BYTES = 2 << 30
STREAM_US = 100000


def _say(**kw):
    print(json.dumps(kw), flush=True)


def _commands():
    """Lines of stdin as they arrive, through a queue: an aggressor polls it between kernels."""
    q = queue.Queue()

    def pump():
        for line in sys.stdin:
            q.put(json.loads(line))
        q.put({"op": "exit"})

    threading.Thread(target=pump, daemon=True).start()
    return q


def victim(launches):
    import torch
    from amdvgpu.ops import mem_latency, ring_build
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seed, rings = 0x3E3F20BE, {}
    for name, nbytes in SIZES.items():
        rings[name] = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
        ring_build(rings[name], (nbytes // 128).bit_length() - 1, seed)
    torch.cuda.synchronize()
    chain_base = 0
    q = _commands()
    _say(ready="victim", cus=cus)
    while True:
        cmd = q.get()
        if cmd["op"] == "exit":
            return 0
        res = {}
        for name, nbytes in SIZES.items():
            runs = []
            for _ in range(launches):
                if nbytes > COLD:
                    # chain 64 b + chain_base of every block b: 1 / 64 of the ring per launch, never the same
                    r = mem_latency(nbytes, nblocks=cus, warm=False, seed=seed, ring=rings[name], chain_base=chain_base % 64)
                    chain_base += 1
                else:
                    r = mem_latency(nbytes, nblocks=cus, warm=True, seed=seed, ring=rings[name])
                runs.append(r)
            res[name] = {"ns": [r["ns_per_load"] for r in runs], "cycles": [r["cycles_per_load"] for r in runs],
                         "cus": len(runs[-1]["cus"]), "steps": runs[-1]["steps"], "chains": runs[-1]["chains"],
                         "laps": runs[-1]["laps"]}
        _say(measured=res)


def aggressor():
    import torch
    from amdvgpu.ops import mem_stream, pattern_fill
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = min(16 * cus, 16384)
    buf = torch.empty(STREAM_BYTES // 4, dtype=torch.int32, device="cuda")
    pattern_fill(buf, 1)
    torch.cuda.synchronize()
    q = _commands()
    _say(ready="aggressor", cus=cus, waves=waves)
    mode, kernels, moved, busy = None, 0, 0, 0.0
    while True:
        try:
            cmd = q.get(block=mode is None)
        except queue.Empty:
            cmd = None
        if cmd and cmd["op"] == "exit":
            return 0
        if cmd and cmd["op"] == "stream":
            mode, kernels, moved, busy = cmd["mode"], 0, 0, 0.0
        if cmd and cmd["op"] == "idle":
            _say(idle=True, mode=mode, kernels=kernels, gbps=moved / busy / 1e9 if busy else 0.0)
            mode = None
        if mode is not None:
            r = mem_stream(buf, mode, waves, STREAM_US, 1 << 20, 1, check=False)
            kernels, moved, busy = kernels + 1, moved + r["bytes"], busy + r["wall_s"]
            if kernels == 1:
                _say(streaming=mode, cus=len(r["cus"]))


class Pod:
    def __init__(self, role, env, limit, extra=()):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--role", role, *extra]
        self.role = role
        self.p = subprocess.Popen(cmd, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def send(self, **kw):
        self.p.stdin.write(json.dumps(kw) + "\n")
        self.p.stdin.flush()

    def read(self, key):
        """The next JSON line with `key`; a child that ended instead stops the whole run."""
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise SystemExit(f"{self.role} pod ended with exit status {self.p.wait()}: stopping")
            if line.startswith("{"):
                msg = json.loads(line)
                if key in msg:
                    return msg


def run(a):
    from amdvgpu.plugin.devices import SysfsBackend
    from amdvgpu.plugin.kubelet_stub import NodeHarness
    from amdvgpu.shim.launcher import apply_contract
    backend = SysfsBackend()
    uuid = backend.devices()[0].uuid
    arms = [("alone", None, 0)] + [(f"{m} x{k}", m, k) for m in ("read", "write") for k in (1, 2, 3)]
    runs, pods = [], []
    with NodeHarness(backend, device_split_count=4, cu_mode=a.cu_mode, workdir=tempfile.mkdtemp(prefix="memi-")) as node:
        try:
            vids = node.vgpu_ids(uuid)[:4]
            envs = [apply_contract(*node.pod([vid])) for vid in vids]
            pods.append(Pod("victim", envs[0], a.limit, ["--launches", str(a.launches)]))
            pods += [Pod("aggressor", env, a.limit) for env in envs[1:]]
            ready = [p.read("ready") for p in pods]
            vic, aggs = pods[0], pods[1:]
            t0 = time.time()
            for rep in range(a.repeats):
                for name, mode, k in arms:
                    for p in aggs[:k]:
                        p.send(op="stream", mode=mode)
                    started = [p.read("streaming") for p in aggs[:k]]
                    vic.send(op="measure")
                    got = vic.read("measured")["measured"]
                    for p in aggs[:k]:
                        p.send(op="idle")
                    idle = [p.read("idle") for p in aggs[:k]]
                    runs.append({"arm": name, "repeat": rep, "t": round(time.time() - t0, 2), "victim": got,
                                 "aggressors": [{"gbps": round(i["gbps"], 1), "kernels": i["kernels"], "cus": s["cus"]}
                                                for i, s in zip(idle, started)]})
                    print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
            for p in pods:
                p.send(op="exit")
            for p in pods:
                if p.p.wait(timeout=60) != 0:
                    raise SystemExit(f"{p.role} pod ended with exit status {p.p.returncode}")
        finally:
            for p in pods:
                if p.p.poll() is None:
                    p.p.kill()
    summary = {}
    for name, _, _ in arms:
        mine = [r for r in runs if r["arm"] == name]
        summary[name] = {"aggressor_gbps": [round(statistics.median(x), 1) for x in
                                            zip(*[[g["gbps"] for g in r["aggressors"]] for r in mine])]}
        for size in SIZES:
            ns = [x["median"] for r in mine for x in r["victim"][size]["ns"]]
            cy = [x["median"] for r in mine for x in r["victim"][size]["cycles"]]
            p90 = [x["p90"] for r in mine for x in r["victim"][size]["ns"]]
            summary[name][size] = {"ns": round(statistics.median(ns), 1), "ns_min": round(min(ns), 1),
                                   "ns_max": round(max(ns), 1), "ns_p90": round(statistics.median(p90), 1),
                                   "cycles": round(statistics.median(cy), 1), "launches": len(ns)}
    for name in summary:
        for size in SIZES:
            summary[name][size]["vs_alone"] = round(summary[name][size]["ns"] / summary["alone"][size]["ns"], 2)
    return {"cu_mode": a.cu_mode, "repeats": a.repeats, "launches": a.launches, "pods": ready, "sizes": SIZES,
            "stream_bytes": STREAM_BYTES, "stream_us": STREAM_US, "summary": summary, "runs": runs}


def table(res):
    md = ["| arm | aggressors GB/s | " + " | ".join(f"{s} ns/load (cycles) | x alone" for s in SIZES) + " |",
          "|---|---|" + "---|---|" * len(SIZES)]
    for name, row in res["summary"].items():
        cells = " | ".join(f"{row[s]['ns']} [{row[s]['ns_min']} .. {row[s]['ns_max']}] ({row[s]['cycles']}) | "
                           f"{row[s]['vs_alone']}" for s in SIZES)
        md.append(f"| {name} | {' + '.join(str(g) for g in row['aggressor_gbps']) or '-'} | {cells} |")
    return "\n".join(md) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--role", default=None, choices=["victim", "aggressor"])
    ap.add_argument("--cu-mode", default="spatial")
    ap.add_argument("--repeats", type=int, default=3, help="times the whole sequence of arms runs (at least 3)")
    ap.add_argument("--launches", type=int, default=3, help="timed launches per ring and arm")
    ap.add_argument("--limit", type=int, default=900, help="seconds every pod process may live")
    ap.add_argument("--json-out")
    ap.add_argument("--md-out")
    a = ap.parse_args()
    if a.role == "victim":
        return victim(a.launches)
    if a.role == "aggressor":
        return aggressor()
    if a.repeats < 3:
        ap.error("--repeats is at least 3")
    res = run(a)
    print(json.dumps(res), flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(res, f, indent=1)
    if a.md_out:
        with open(a.md_out, "w") as f:
            f.write(table(res))
    print(table(res), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
