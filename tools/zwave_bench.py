#!/usr/bin/env python3
"""Z-Wave R2 receive path throughput on one MI355X (bench.py's workloads are the BTLE / 802.15.4 ones; this is the
separate measurement of SNOUT_PROTO_ZWAVE).

The capture: 2^28 cf32 samples at 800 ksps built on the device from distinct tiles -- eight seeded synthetic 2^22-sample
captures, each placed eight times with its own constant phase rotation.  Every call processes the whole capture
(submit / collect, two in flight); ms per call from HIP events on the stream, the dominant kernel (zw_front) from the
library's own events.  parity_in_run: the records of the first 2^20 samples of the same device buffer against
tests/zwave_ref.py (lane mode, every field).  Prints one JSON line.

    python tools/zwave_bench.py --steps 10 --warmup 2
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=28)
    a = ap.parse_args()
    import torch
    from snout_amd import _ffi, zwave
    from snout_amd.rx import SnoutRx
    from oracle import oracle_py
    import zwave_ref as ref

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = 1 << a.log2n
    tile = 1 << 22
    x = torch.empty(2 * n, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(28)
    tiles = [torch.from_numpy(zwave.capture(tile, seed=1000 + s)[0]).to(dev) for s in range(8)]
    for k in range(n // tile):
        rot = np.exp(1j * rng.uniform(0, 2 * np.pi))
        t = tiles[k % 8] * torch.tensor(complex(rot), dtype=torch.complex64, device=dev)
        x[2 * k * tile:2 * (k + 1) * tile] = torch.view_as_real(t).reshape(-1)
    torch.cuda.synchronize()

    rx = SnoutRx(proto=_ffi.PROTO_ZWAVE, device=0)
    st = torch.cuda.current_stream()
    frames = 0
    for _ in range(a.warmup):
        frames = len(rx.process(x))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    got = 0
    for i in range(a.steps):
        rx.submit(x)
        if i >= 1:
            got = len(rx.collect())
    got = len(rx.collect())
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.steps
    hist = rx.profile_history()
    dom = float(np.median(hist[-a.steps:]))
    # parity on a subset of the same device capture
    sub = x[:2 * (1 << 20)]
    g = rx.process(sub)
    xs = sub.cpu().numpy().view(np.complex64)
    rx.close()
    want, _, _ = ref.receive(xs, oracle_py.zb_mmse_taps())
    ok = len(g) == len(want) > 0
    for p, w in zip(g, want):
        ok = ok and all(int(p[k]) == int(w[k]) for k in ("sample_index", "proto", "channel", "len", "crc_ok", "pdu_type", "aux"))
        ok = ok and bytes(p["bytes"][:w["len"]]) == w["bytes"]
    print(json.dumps({"workload": "zwave_r2_800k", "samples_per_call": n, "steps": a.steps, "ms_per_call": round(ms, 3),
                      "gsamples_per_s": round(n / ms / 1e6, 3), "dominant": "zw_front", "ms_dominant": round(dom, 3),
                      "frames": frames, "frames_last_call": got, "parity_in_run": bool(ok),
                      "parity_frames": len(want)}))


if __name__ == "__main__":
    main()
