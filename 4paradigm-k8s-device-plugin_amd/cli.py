"""``python -m amdvgpu <command>`` — one entry point for the node and for debugging.

    plugin   [flags]                     run the device plugin (same flags as plugin.main)
    monitor  [--root DIR] [--port N]     Prometheus metrics + control API over regions
    run      [--memory 16g] [--cu 25] [--cu-range 0-64] [--oversubscribe] -- CMD...
                                         run CMD as a vGPU 'container' under the shim
    region   PATH [show|suspend|resume|set-limit DEV SIZE|set-cu DEV PCT|reclaim]
    devices  [--backend auto|sysfs|amdsmi|fake]   print the discovered GPUs as JSON
    memprobe [--sizes 16k,1m,64m,2g] [--json]     load latency per working set and stream GB/s
                                         of the GPU this process sees (under `run`: the slice)
"""
import argparse
import json
import sys


def _run(argv):
    from .shim.launcher import cleanup_region, run, vgpu_env
    from .utils.sizes import parse_size
    ap = argparse.ArgumentParser(prog="amdvgpu run")
    ap.add_argument("--memory", default=None, help="HBM quota, e.g. 16g")
    ap.add_argument("--hbm", default=None, help="HBM-resident share (with --oversubscribe)")
    ap.add_argument("--cu", type=int, default=None, help="CU share in percent")
    ap.add_argument("--cu-range", default=None, help="logical CU range b-e")
    ap.add_argument("--cu-mode", default=None, choices=["auto", "spatial", "temporal", "both", "off"])
    ap.add_argument("--oversubscribe", action="store_true")
    ap.add_argument("--region", default=None, help="shared region file (default: a fresh /tmp file)")
    ap.add_argument("--keep-region", action="store_true")
    ap.add_argument("cmd", nargs=argparse.REMAINDER)
    a = ap.parse_args(argv)
    cmd = a.cmd[1:] if a.cmd and a.cmd[0] == "--" else a.cmd
    if not cmd:
        ap.error("no command given")
    extra = {}
    if a.hbm:
        extra["VGPU_DEVICE_HBM_LIMIT_0"] = f"{parse_size(a.hbm) >> 20}m"
    rng = tuple(int(x) for x in a.cu_range.split("-")) if a.cu_range else None
    c = vgpu_env(mem_limit=parse_size(a.memory) if a.memory else None, cu_limit=a.cu, cu_range=rng,
                 cu_mode=a.cu_mode, oversubscribe=a.oversubscribe, shared_cache=a.region, extra=extra)
    try:
        return run(cmd, c).returncode
    finally:
        if not a.keep_region and not a.region:
            cleanup_region(c)


def _region(argv):
    from .shim.region import Region
    from .utils.sizes import parse_size
    if not argv:
        print("usage: amdvgpu region PATH [show|suspend|resume|set-limit DEV SIZE|set-cu DEV PCT|reclaim]")
        return 2
    r = Region(argv[0])
    op = argv[1] if len(argv) > 1 else "show"
    if op == "show":
        print(json.dumps(r.snapshot(), indent=1))
    elif op == "suspend":
        r.suspend_all()
    elif op == "resume":
        r.resume_all()
    elif op == "set-limit":
        r.set_memory_limit(int(argv[2]), parse_size(argv[3]))
    elif op == "set-cu":
        r.set_cu_limit(int(argv[2]), int(argv[3]))
    elif op == "reclaim":
        print(r.reclaim())
    else:
        print(f"unknown region op {op}", file=sys.stderr)
        return 2
    return 0


def _devices(argv):
    from .plugin.devices import detect_backend
    ap = argparse.ArgumentParser(prog="amdvgpu devices")
    ap.add_argument("--backend", default="auto")
    ap.add_argument("--fake", default=None)
    a = ap.parse_args(argv)
    be = detect_backend(a.backend, a.fake)
    devs = be.devices() if be else []
    print(json.dumps([d.to_dict() for d in devs], indent=1))
    return 0


def _memprobe(argv):
    """Pointer-chase latency per working set (one lane per wave, one wave per CU the process
    sees) and the read and write bandwidth of a 100 ms stream, alone in this process. It runs in
    whatever environment it is started in: under ``amdvgpu run --cu 25 -- ...`` it measures the
    slice."""
    from .utils.sizes import parse_size
    ap = argparse.ArgumentParser(prog="amdvgpu memprobe")
    ap.add_argument("--sizes", default="16k,1m,64m,2g", help="working sets, powers of two from 256 to 4g")
    ap.add_argument("--stream-bytes", default="1g", help="buffer of the timed stream")
    ap.add_argument("--stream-ms", type=int, default=100)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    sizes = [parse_size(x) for x in a.sizes.split(",") if x]
    for n in sizes:
        if n & (n - 1) or not 256 <= n <= 4 << 30:
            ap.error(f"working set {n} is no power of two between 256 bytes and 4 GiB")
    stream_bytes = parse_size(a.stream_bytes)
    if not 0 <= a.stream_ms <= 1000:
        ap.error("--stream-ms is 0..1000")
    import torch
    from .ops import mem_latency, mem_stream, pattern_fill
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"cus": cus, "latency": [], "stream": {}}
    for n in sizes:
        r = mem_latency(n)
        r["cus"] = len(r["cus"])
        res["latency"].append(r)
        torch.cuda.empty_cache()
    buf = torch.empty(stream_bytes // 4, dtype=torch.int32, device="cuda")
    waves = min(16 * cus, 16384)
    pattern_fill(buf, 1)
    for mode in ("read", "write"):
        mem_stream(buf, mode, waves, 0, 1, 1, check=False)              # one untimed pass
        r = mem_stream(buf, mode, waves, a.stream_ms * 1000, 1 << 20, 1, check=False)
        res["stream"][mode] = {"gbps": r["gbps"], "bytes": r["bytes"], "wall_s": r["wall_s"], "waves": waves,
                               "passes_min": int(r["passes"].min()), "passes_max": int(r["passes"].max()),
                               "cus": len(r["cus"])}
    if a.json:
        print(json.dumps(res))
        return 0
    print(f"{cus} CUs visible; one lane per wave, one wave per CU; median (p10 .. p90) over the chains")
    for r in res["latency"]:
        ns, cy = r["ns_per_load"], r["cycles_per_load"]
        print(f"  {r['bytes']:>11} B  {ns['median']:8.1f} ns ({ns['p10']:.1f} .. {ns['p90']:.1f})  "
              f"{cy['median']:8.1f} cycles ({cy['p10']:.1f} .. {cy['p90']:.1f})  per load; {r['chains']} chains x "
              f"{r['steps']} steps on {r['cus']} CUs, {r['laps']:.3g} laps")
    for mode, r in res["stream"].items():
        print(f"  stream {mode:<5} {r['gbps']:8.1f} GB/s  ({r['bytes']} B in {r['wall_s'] * 1e3:.1f} ms, {r['waves']} waves "
              f"on {r['cus']} CUs, {r['passes_min']}..{r['passes_max']} passes)")
    return 0


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] in ("-h", "--help"):
        print(__doc__)
        return 0
    cmd, rest = argv[0], argv[1:]
    if cmd == "plugin":
        from .plugin.main import main as plugin_main
        return plugin_main(rest)
    if cmd == "monitor":
        from .plugin.monitor import main as monitor_main
        return monitor_main(rest)
    if cmd == "run":
        return _run(rest)
    if cmd == "region":
        return _region(rest)
    if cmd == "devices":
        return _devices(rest)
    if cmd == "memprobe":
        return _memprobe(rest)
    print(f"unknown command {cmd!r}\n{__doc__}", file=sys.stderr)
    return 2
