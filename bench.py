#!/usr/bin/env python3
"""bench.py — benchmark of the MI355X IQ->packets receive path on BASELINE.json's metric.

    python bench.py --gpus 1 --steps K --warmup W
        headline: cfg #3 (BASELINE.json configs[2]): 80 Msps wideband capture -> 40-channel polyphase
        channelizer -> BTLE demod + access-address correlate + de-whiten/CRC on every channel, 8e8
        cf32 samples (10 s of band) resident in HBM.  `roofline` is the channelizer kernel
        (HBM fraction of the 8 TB/s spec peak, of the read rate measured in this process, and the
        fp32 FLOP fraction); `cpu_baseline` times the CPU oracle on a bounded sample with 1 thread
        and with all host cores.  `other_workloads` carries cfg #2 (single-channel BTLE, 1e9
        samples), cfg #4 (16-channel 802.15.4, 3.2e8), single-channel 802.15.4 (1e9) and cfg #5 on
        this one GPU, measured in the same process under the same contract.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
        the SAME workload on every rank (weak scaling: rank r holds its own 8e8-sample capture segment, the
        r-th 10 s of an N x 10 s capture; segments are independent, no sample ever crosses ranks), the decoded
        records of every step gathered to rank 0 by one RCCL all_gather, overlapped with the next step, all inside
        the timed region: value(N) / (N value(1)) is the scaling efficiency.  `other_workloads.cfg5` carries
        BASELINE.json configs[4] on the same N ranks: the BTLE 40-channel and the 802.15.4 16-channel wideband
        scans concurrently, each capture cut into segments of 2^24 input samples that overlap by the longest
        packet, segment i -> rank i mod N, records gathered per step over RCCL and de-duplicated on rank 0's GPU
        (`--workload cfg5` makes it the headline).

`--workload X` runs one workload alone (N = 1: that workload is the headline; N > 1: every rank
processes its own copy of it, records gathered per step).

A "step" is one pass of the whole receive path over the resident capture, packet records landed in
host memory (rank 0's for N > 1).  Prints ONE JSON line (rank 0).  Kernel durations are HIP-event
pairs recorded on the kernel's own stream during the timed steps.

Captures (round 6): every capture cycles through TILES = 32 independently seeded, noise-free tiles of the workload's
traffic (narrowband tiles from snout_amd.synth on the host, wideband ones composed on the device by the same upsampler:
wideband_tile_dev) plus independent AWGN on every sample -- a statistic over a capture counts thousands of DISTINCT packets.
Checks outside the timed region: `parity_in_run` (the HIP path's records == the CPU oracle's, every field and byte: whole
captures at N = 1; cfg #5 at every N -- every rank's oracle records gathered to rank 0), `frames_lost_vs_sequential` with
`fidelity_modes` for the 802.15.4 lines (the default lanes + frame repair against ONE sequential lane per channel, the
reference's receiver).  `frac` prices the dominant kernel's event duration, `step_frac` the whole step.

`--dump-outputs DIR` (rank 0) writes the records the timed path handed its caller in the LAST timed step -- rank 0's
gathered records at N > 1, both scans' for cfg5 -- as DIR/<name>_<field>.npy (see dump_outputs), so that two builds can be
compared output for output: the captures depend on the arguments alone (seeded tiles and noise).
"""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "complex-IQ Msamples/s through channelize+demod; decoded pkts/s; HBM GB/s %peak"   # BASELINE.json
HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
FP32_PEAK_TFLOPS = 157.3        # MI355X fp32 vector peak (same guide)
SIGMA = 0.05
SEG = 1 << 24                   # cfg #5 segment length in input samples

# flop per input sample of the channelizer: (M P 4 + 5 M log2 M) / D
PFB_FLOP = {40: (40 * 16 * 4 + 5 * 40 * np.log2(40)) / 20, 16: (16 * 16 * 4 + 5 * 16 * 4) / 8}

WORKLOADS = {
    # name: (proto, n_channels, channel, samples per GPU, gathered record bytes, description)
    "cfg2": (0, 1, 37, 1e9, 96,
             "cfg2: single-channel BTLE (ch37) GFSK demod + access-address correlate + dewhiten/CRC"),
    "cfg3": (0, 40, 0, 8e8, 96,
             "cfg3: 80 Msps wideband -> 40-channel polyphase channelizer -> BTLE receive on every channel"),
    "cfg4": (1, 16, 0, 3.2e8, 160,
             "cfg4: 32 Msps wideband -> 16-channel polyphase channelizer -> 802.15.4 receive on every channel"),
    "zigbee1": (1, 1, 11, 1e9, 160,
                "single-channel 802.15.4 (ch11): discriminator + DC removal + M&M clock recovery + packet sink"),
}
CFG5_DESCR = ("cfg5: BTLE 40-channel (80 Msps) and 802.15.4 16-channel (32 Msps) wideband scans concurrently, "
              "10 s of each band per GPU in 2^24-sample overlapping segments, segment i -> rank i mod N")

# bounded CPU samples: about 10 s of single-thread oracle time per leg
CPU_SAMPLES = {"cfg2": 2.5e8, "cfg3": 40 * (1 << 21), "cfg4": 16 * (1 << 21), "zigbee1": 1 << 26}
CPU_SOURCE = {"cfg2": "oracle/oracle_btle.c", "cfg3": "oracle/oracle_pfb.c + oracle_btle.c",
              "cfg4": "oracle/oracle_pfb.c + oracle_zigbee.c", "zigbee1": "oracle/oracle_zigbee.c"}


# ------------------------------------------------------------------------------------------------
# synthetic captures
# ------------------------------------------------------------------------------------------------
TILES = 32                      # distinct seeded tiles of traffic per capture


def make_tile(workload: str, seed: int, n_tile: int = 0):
    """ONE noise-free host tile of the workload's traffic and its truth list (numpy throughout: tests and dev tools)."""
    from snout_amd import synth
    if workload == "cfg2":
        return synth.btle_capture(n_tile or (1 << 22), channel=37, seed=seed, noise=False)
    if workload == "zigbee1":
        return synth.zigbee_capture(n_tile or (1 << 19), channel=11, seed=seed, noise=False)     # (32 tiles = the 2^24-sample prefix one sequential lane is run on)
    if workload == "cfg3":
        return synth.wideband_capture(0, n_tile or 40 * (1 << 16), seed=seed, sigma=0.0)
    if workload == "cfg4":
        return synth.wideband_capture(1, n_tile or 16 * (1 << 17), seed=seed, sigma=0.0)
    raise SystemExit(f"unknown workload {workload}")


_UP_FILTERS = {}


def _upsample_dev(x, up: int):
    """complex64 [n] -> complex64 [n up] on x's device: zero-stuffing + the windowed-sinc low-pass of
    scipy.signal.resample_poly(x, up, 1) (firwin(20 up + 1, 1 / up, kaiser 5.0) x up), as one polyphase conv1d."""
    import torch
    key = (up, str(x.device))
    if key not in _UP_FILTERS:
        from scipy.signal import firwin
        half = 10 * up
        h = firwin(2 * half + 1, 1.0 / up, window=("kaiser", 5.0)) * up
        w = np.zeros((up, 21), dtype=np.float32)
        for p in range(up):                                 # y[up q + p] = sum_j x[q - j] h[p + half + up j], j = 10 - t
            for t in range(21):
                idx = p + half + up * (10 - t)
                if 0 <= idx <= 2 * half:
                    w[p, t] = h[idx]
        _UP_FILTERS[key] = torch.from_numpy(w).to(x.device)[:, None, :]
    w = _UP_FILTERS[key]
    xr = torch.view_as_real(x).transpose(0, 1).contiguous()[:, None, :]          # [2 (re, im), 1, n]
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xr, (10, 10)), w)      # [2, up, n]
    y = y.permute(0, 2, 1).reshape(2, -1)
    return torch.complex(y[0], y[1])


def wideband_tile_dev(proto: int, n_samples: int, seed: int, device):
    """snout_amd.synth.wideband_capture(proto, n_samples, seed, sigma=0) with the compositor on the device: every bin's
    4 Msps traffic stream comes from the same host generators with the same seeds (so the truth list is the same), the
    upsampling to the wideband rate, the shift to the bin centre and the sum run in torch (f32 instead of the host's
    complex128 filter: equal to ~1e-6 of full scale, tests/test_bench_host.py).  Returns (complex64 tensor, truth)."""
    import torch
    from snout_amd import synth
    M = 40 if proto == 0 else 16
    up = M // 2
    n_ch = n_samples // up
    x = torch.zeros(n_ch * up, dtype=torch.complex64, device=device)
    ang = torch.arange(M, device=device, dtype=torch.float64) * (2.0 * np.pi / M)
    rot_tab = torch.complex(torch.cos(ang), torch.sin(ang)).to(torch.complex64)
    t = torch.arange(n_ch * up, device=device, dtype=torch.int64)
    truth = []
    for b in range(M):
        if proto == 0:
            nb, tr = synth.btle_capture(n_ch, channel=synth.btle_bin_channel(b), seed=seed * 1000 + b, noise=False)
        else:
            nb, tr = synth.zigbee_capture(n_ch, channel=synth.zigbee_bin_channel(b), seed=seed * 1000 + b, noise=False,
                                          slot_phase=b & 1)
        wb = _upsample_dev(torch.from_numpy(nb).to(device), up)
        x += wb * rot_tab[(b * t) % M]
        truth.extend(tr)
    return x, truth


def make_tiles(workload: str, seed: int, device, n_tile: int = 0, k: int = TILES):
    """K distinct noise-free tiles of the workload's traffic on the device (float32 [k, 2 L], interleaved) and their truth
    lists.  VERDICT r5 item 4a: one tile repeated carried "a few dozen distinct frames"; a capture now cycles through k
    independently seeded tiles (tile t: seed 100 seed + t), so that a statistic over it counts thousands of distinct
    packets.  Narrowband tiles come from the host generators, wideband ones from wideband_tile_dev."""
    import torch
    tiles, truths = [], []
    for t in range(k):
        sd = 100 * seed + t
        if workload in ("cfg2", "zigbee1"):
            h, tr = make_tile(workload, sd, n_tile)
            d = torch.from_numpy(np.ascontiguousarray(h).view(np.float32)).to(device)
        else:
            c, tr = wideband_tile_dev(0 if workload == "cfg3" else 1, n_tile or (40 * (1 << 16) if workload == "cfg3" else 16 * (1 << 17)),
                                      sd, device)
            d = torch.view_as_real(c).reshape(-1)
        tiles.append(d)
        truths.append(tr)
    return torch.stack(tiles), truths


def fill_capture(x, g0: int, tiles, gen) -> None:
    """x (float32 [2 n], on the device) <- samples [g0, g0 + n) of the VIRTUAL capture whose tile g (L samples each) is
    tiles[g mod K], plus independent AWGN on every sample (generated on the device)."""
    import torch
    L = tiles.shape[1] // 2
    n = x.numel() // 2
    pos = 0
    while pos < n:
        g, off = divmod(g0 + pos, L)
        m = min(L - off, n - pos)
        seg = x[2 * pos:2 * (pos + m)]
        torch.randn(seg.shape, generator=gen, device=x.device, out=seg)
        seg.mul_(SIGMA).add_(tiles[g % tiles.shape[0]][2 * off:2 * (off + m)])
        pos += m


def resident_capture(tiles, n_samples: int, seed: int, device, first_sample: int = 0):
    """Capture in HBM: samples [first_sample, first_sample + n_samples) of the virtual capture made of `tiles` (a
    [K, 2 L] device tensor from make_tiles, or one host tile) plus independent AWGN."""
    import torch
    if isinstance(tiles, np.ndarray):
        tiles = torch.from_numpy(np.ascontiguousarray(tiles).view(np.float32)).to(device)[None, :]
    x = torch.empty(2 * n_samples, dtype=torch.float32, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(1000 + seed)
    fill_capture(x, first_sample, tiles, g)
    torch.cuda.synchronize(device)
    return x


def truth_in(truths, tile_len: int, n_samples: int, first_sample: int = 0):
    """(whole tiles' packets, the set of payloads) of samples [first_sample, first_sample + n_samples) of the virtual
    capture: packets of tiles that lie wholly inside it."""
    g_lo = -(-first_sample // tile_len)
    g_hi = (first_sample + n_samples) // tile_len
    return sum(len(truths[g % len(truths)]) for g in range(g_lo, g_hi))


def expected_ok(workload: str, truths, tile_len: int, n_samples: int) -> int:
    whole = truth_in(truths, tile_len, n_samples)
    if workload == "cfg2":
        full = n_samples // tile_len
        rem = n_samples - full * tile_len
        return whole + sum(1 for p in truths[full % len(truths)] if p.sample_index + 1600 < rem)
    # wideband truth indices are at the channel rate: count whole tiles only.  cfg4: the synthetic
    # 2 MHz raster makes adjacent 802.15.4 channels overlap spectrally; their traffic is slotted so
    # that neighbours never transmit together, but a neighbour's leakage still drags the receiver's
    # DC estimate before some frames: ~93 % decode on the oracle and on the GPU alike
    return int((0.8 if workload == "cfg4" else 0.9) * whole)


def quantise(x, fmt: int):
    """What an SDR's ADC path would have delivered: full scale = 1.25 x the largest component."""
    import torch
    bits = 7 if fmt == 1 else 15
    scale = float(1 << bits) / (1.25 * float(x.abs().max()))
    xi = torch.empty(x.shape, dtype=torch.int8 if fmt == 1 else torch.int16, device=x.device)
    step = 1 << 26
    for lo in range(0, x.numel(), step):
        xi[lo:lo + step] = (x[lo:lo + step] * scale).round_().clamp_(-(1 << bits), (1 << bits) - 1)
    return xi


# ------------------------------------------------------------------------------------------------
# CPU baseline (the oracle: test infrastructure, here only as the thing timed beside the GPU)
# ------------------------------------------------------------------------------------------------
def cpu_model() -> str:
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_leg(host: np.ndarray, workload: str, threads: int, passes: int):
    from oracle import oracle_py
    oracle_py.set_threads(threads)
    best, n_pk = None, 0
    for _ in range(passes):
        t0 = time.perf_counter()
        if workload == "cfg2":
            pk = (oracle_py.narrowband_parallel(host, 0, 37) if threads > 1
                  else oracle_py.btle_segment(host, channel=37, cap=max(1024, host.size // 4096))[0])
        elif workload == "zigbee1":
            pk = (oracle_py.narrowband_parallel(host, 1, 11) if threads > 1
                  else oracle_py.zigbee_segment(host, channel=11))
        elif threads > 1:
            M = 40 if workload == "cfg3" else 16            # ~4 segments per thread, each a whole serial chain
            seg = max(M * 8192, (host.size // 2 // (4 * threads)) // M * M)
            pk = oracle_py.wideband_parallel(host, 0 if workload == "cfg3" else 1, seg)
        else:
            pk = oracle_py.wideband_segment(host, proto=0 if workload == "cfg3" else 1)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        n_pk = len(pk)
    oracle_py.set_threads(1)
    return best, n_pk, pk


def cpu_baseline(x_dev, workload: str, n_sample: int):
    """Two legs on the first n_sample samples of the resident capture: the scalar port on one
    thread, and the same oracle with OpenMP over output times / channels / segments on all cores."""
    from oracle import oracle_py
    oracle_py.lib()
    host = x_dev[:2 * n_sample].cpu().numpy()
    if host.dtype != np.float32:
        host = oracle_py.from_int(host)     # the oracle's definition of integer input (untimed)
    ncores = oracle_py.hw_threads()
    t1, n_pk, pk1 = cpu_leg(host, workload, 1, passes=2)
    tall, n_pk_all, _ = cpu_leg(host, workload, ncores, passes=3)
    if workload in ("cfg2", "cfg3"):        # BTLE: the seams lose nothing (802.15.4 segments restart the DC filter)
        assert abs(n_pk - n_pk_all) <= max(4, n_pk // 50), (n_pk, n_pk_all)
    return {"value": n_sample / t1 / 1e6, "unit": "Msamples/s", "cores": 1, "kind": "port",
            "sample": "first %.3g samples of the %s capture, %s, gcc -O3 -march=x86-64-v3, best of 2 passes"
                      % (n_sample, workload, CPU_SOURCE[workload]),
            "all_cores": {"value": n_sample / tall / 1e6, "unit": "Msamples/s", "cores": ncores,
                          "how": "same oracle, one OpenMP task per overlapping segment (~4 per thread), each the "
                                 "whole serial chain over every channel; best of 3 passes"},
            "nproc": os.cpu_count(), "cpu_model": cpu_model(), "packets_in_sample": int(n_pk)}, pk1


# ------------------------------------------------------------------------------------------------
# parity in the same run: the HIP path and the oracle on the same prefix of the capture
# ------------------------------------------------------------------------------------------------
PARITY_FIELDS = ("sample_index", "proto", "channel", "len", "crc_ok", "lqi", "pdu_type", "flags", "aux")
# workloads whose WHOLE capture the oracle decodes in seconds to tens of seconds on the GPU box's host cores (as one
# segment: all threads inside the channelizer, then one per bin; cfg2: the scalar loop, ~17 s per 1e9 samples; zigbee1: the
# discriminator and the lanes' loops over all threads, stitching and the sinks on one)
PARITY_FULL = ("cfg2", "cfg3", "cfg4", "zigbee1")


def oracle_records(x_dev, workload: str, n_sample: int):
    """The oracle's records for the first n_sample samples, as ONE segment (all host threads inside the
    channelizer / across the bins: same records as with one thread, sooner)."""
    from oracle import oracle_py
    host = x_dev[:2 * n_sample].cpu().numpy()
    if host.dtype != np.float32:
        host = oracle_py.from_int(host)
    oracle_py.set_threads(oracle_py.hw_threads())
    try:
        if workload == "cfg2":
            return oracle_py.btle_segment(host, channel=37, cap=max(1024, host.size // 4096))[0]
        if workload == "zigbee1":
            return oracle_py.zigbee_segment(host, channel=11)
        return oracle_py.wideband_segment(host, proto=0 if workload == "cfg3" else 1)
    finally:
        oracle_py.set_threads(1)


def parity_in_run(x_dev, workload: str, n_sample: int, device, fmt: int, want=None, got=None):
    """What the reference's consumer keeps are the decoded records (snout/core/message.py:226 keeps the CRC0
    lines): the GPU's record set on the first n_sample samples (the whole capture for PARITY_FULL workloads) must EQUAL
    the oracle's -- every field and every byte.  ``got``: the HIP path's records of exactly those samples, if the
    caller has them already."""
    from snout_amd.rx import SnoutRx
    proto, n_ch, channel = WORKLOADS[workload][:3]
    t0 = time.perf_counter()
    if want is None:
        want = oracle_records(x_dev, workload, n_sample)
    t_oracle = time.perf_counter() - t0
    if got is None:
        with SnoutRx(proto=proto, channel=channel, n_channels=n_ch, device=device.index, sample_format=fmt) as rx:
            got = rx.process(x_dev[:2 * n_sample]).copy()

    def canon(r):
        return r[np.lexsort((r["len"], r["sample_index"], r["channel"]))]
    equal = len(got) == len(want)
    if equal:
        a, b = canon(got), canon(want)
        equal = all(np.array_equal(a[f], b[f]) for f in PARITY_FIELDS) and np.array_equal(a["bytes"], b["bytes"])
    assert equal, f"{workload}: the GPU's records on the first {n_sample} samples differ from the oracle's ({len(got)} vs {len(want)})"
    return {"workload": workload, "samples": int(n_sample), "whole_capture": bool(n_sample * 2 == x_dev.numel()),
            "records": int(len(want)), "crc_ok_records": int(want["crc_ok"].sum()), "equal": True, "oracle_s": round(t_oracle, 2),
            "compared": "every record field and byte, set equality after sorting by (channel, sample_index), against the CPU oracle"}


FIDELITY_SHAPES = ((16384, 8192),)      # lane shapes reported beside the default one (fidelity_modes)


# ------------------------------------------------------------------------------------------------
# --dump-outputs: the last timed step's records, for comparing two builds output for output
# ------------------------------------------------------------------------------------------------
DUMP_ROW_BYTES = 60_000_000     # .npy payload of all outputs together (the headers come on top: under 64 MB in all)
DUMP_SEED = 20250101            # the rows kept when an output is larger: the same rows for the same record count
# the order records are written in: the library's order within a step is not part of its contract (parity_in_run sorts too)
DUMP_ORDER = ("channel", "sample_index", "len", "proto", "crc_ok", "lqi", "pdu_type", "flags", "aux")


def owned_records(parts):
    """One PKT_DTYPE array that owns its memory, from record arrays or wire-format views into pinned buffers."""
    from snout_amd import dist as sdist
    return np.concatenate([np.zeros(0, dtype=_pkt_dtype())] + [sdist.widen_records(np.asarray(p)) for p in parts])


def dump_outputs(path: str, outputs: dict) -> dict:
    """Write every {name: records} as <name>_<field>.npy, float64 [n] (every integer field is exact in it), one per field
    but the payload, <name>_bytes.npy, float32 [n, 136], and <name>_count.npy, float64 [1]: the records before any
    sampling.  Rows in DUMP_ORDER.  When the rows of all outputs exceed DUMP_ROW_BYTES, every output keeps the same fixed
    fraction of its rows, drawn by a generator seeded with DUMP_SEED (kept in DUMP_ORDER)."""
    dt = _pkt_dtype()
    fields = [f for f in dt.names if f != "bytes"]
    row = 8 * len(fields) + 4 * dt["bytes"].shape[0]
    total = sum(len(r) for r in outputs.values())
    frac = min(1.0, DUMP_ROW_BYTES / (row * total)) if total else 1.0
    os.makedirs(path, exist_ok=True)
    info = {"dir": path, "order": list(DUMP_ORDER), "records": {}, "rows_written": {}}
    for name, rec in outputs.items():
        rec = rec[np.lexsort(tuple(rec[f] for f in reversed(DUMP_ORDER)))]
        n = len(rec)
        k = n if frac >= 1.0 else int(n * frac)
        if k < n:
            rec = rec[np.sort(np.random.default_rng(DUMP_SEED).choice(n, k, replace=False))]
        np.save(os.path.join(path, name + "_count.npy"), np.array([n], dtype=np.float64))
        for f in fields:
            np.save(os.path.join(path, "%s_%s.npy" % (name, f)), rec[f].astype(np.float64))
        np.save(os.path.join(path, name + "_bytes.npy"), rec["bytes"].astype(np.float32))
        info["records"][name] = n
        info["rows_written"][name] = k
    return info


def lost_vs_sequential(x_dev, workload: str, n_sample: int, device, fmt: int, shapes=()):
    """802.15.4 workloads: the DEFAULT decode (lanes + frame repair) against ONE sequential lane per channel -- the
    reference's receiver (Zigbee_rx/top_block.py:67,69: one clock_recovery_mm_ff / packet_sink loop per channel) -- both on
    the GPU, on the first n_sample samples of the capture the steps are timed on (outside the timed region).  One lane on
    the GPU is the oracle's one lane record for record (tests/test_zigbee_gpu.py, test_fullsize_gpu.py).  Frames = FCS-ok
    records; a frame matches if channel and bytes agree and the start is within 8 samples.  ``shapes``: further
    (core, warm-up) lane shapes compared with the same sequential records -> "fidelity_modes" (what
    exactness costs), together with the measured rate of the one-lane decode itself."""
    import collections
    import torch
    from snout_amd.rx import SnoutRx
    proto, n_ch, channel = WORKLOADS[workload][:3]
    assert proto == 1
    part = x_dev[:2 * n_sample]
    t0 = time.perf_counter()
    with SnoutRx(proto=proto, channel=channel, n_channels=n_ch, device=device.index, sample_format=fmt, zb_core=1 << 24) as rx:
        one = rx.process(part).copy()           # (first call: allocations)
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        rx.process(part, copy=False)
        t_one = time.perf_counter() - t1

    def keys(a):
        a = a[a["crc_ok"] == 1]
        return [(int(c), bytes(b[:l]), int(i)) for c, i, l, b in zip(a["channel"], a["sample_index"], a["len"], a["bytes"])]

    def missing(A, B):
        d = collections.defaultdict(list)
        for c, b, i in B:
            d[(c, b)].append(i)
        return sum(1 for c, b, i in A if not any(abs(i - u) <= 8 for u in d.get((c, b), [])))
    ko = keys(one)

    def against(core, warm):
        with SnoutRx(proto=proto, channel=channel, n_channels=n_ch, device=device.index, sample_format=fmt, zb_core=core, zb_warmup=warm) as rx:
            got = rx.process(part).copy()
        kg = keys(got)
        lost, extra = missing(ko, kg), missing(kg, ko)
        return {"frames": len(kg), "lost": lost, "extra": extra, "frac_lost": lost / max(1, len(ko)), "frac_extra": extra / max(1, len(ko)),
                "frac_lost_plus_extra": (lost + extra) / max(1, len(ko)), "repaired": int(((got["flags"] & 8) != 0).sum())}
    d = against(0, 0)
    res = {"samples": int(n_sample), "sequential_frames": len(ko), "distinct_sequential_frames": len({(c, b) for c, b, _ in ko}),
           "default_frames": d["frames"], "lost": d["lost"], "extra": d["extra"],
           "frac_lost": d["frac_lost"], "frac_extra": d["frac_extra"], "frac_lost_plus_extra": d["frac_lost_plus_extra"],
           "repaired": d["repaired"], "lane_shape": "%s (default) + frame repair" % ("6144 / 3072" if n_ch > 1 else "6144 / 1024"),
           "sequential": "zb_core >= the prefix: one lane per channel on the GPU (== the oracle's, == Zigbee_rx/top_block.py:67,69)"}
    if shapes:
        res["fidelity_modes"] = {"%d / %d" % (c, w): against(c, w) for c, w in shapes}
        res["fidelity_modes"]["one lane per channel"] = {"lost": 0, "extra": 0, "Msamples_per_s": n_sample / t_one / 1e6,
                                                         "note": "the reference's receiver itself (zb_core >= the call): one serial loop per channel"}
    res["seconds"] = round(time.perf_counter() - t0, 2)
    return res


def _pkt_dtype():
    from snout_amd._ffi import PKT_DTYPE
    return PKT_DTYPE


def reserved_cus(world: int, fake: int) -> int:
    """Compute units the channelizer's persistent grid leaves free (cfg.reserved_cus).

    N = 1 (and the one-GPU rehearsal of rank 0's load): 0 -- measured (profiles/r4_fake_world.txt, r6_fake_world.txt): reserving
    costs what it reserves (8 CUs: + 0.8 % on the headline step, 16: + 3 %) and buys nothing, because everything rank 0 runs
    for the exchange there (pack, de-duplication, blit downloads) is work of ITS OWN that fits between or beside two launches.

    N > 1: 8, by construction -- it cannot be measured on a one-GPU pool.  An RCCL collective is a kernel on EVERY rank that
    completes only while its peers' kernels run too, and a rank's kernel is dispatched when that rank has a CU free: with
    every CU held by a persistent channelizer workgroup that is the ~0.1 ms between two launches, at a phase of the 2.5 ms
    step that no other rank shares.  A collective kernel that started in rank A's gap then holds its CUs, spinning, until
    rank B reaches its own gap -- across A's next channelizer launch, whose last workgroups wait for those CUs and finish a
    launch late.  Eight CUs (one per RCCL channel: NCCL_MAX_NCHANNELS=8 below) left out of the grid let the collectives run
    whenever they are launched.  SNOUT_BENCH_RESERVED_CUS overrides."""
    e = os.environ.get("SNOUT_BENCH_RESERVED_CUS")
    if e is not None:
        return int(e)
    return 8 if world > 1 else 0


# ------------------------------------------------------------------------------------------------
# one workload on one handle, pipelined submit / collect
# ------------------------------------------------------------------------------------------------
def run_workload(name: str, n: int, steps: int, warmup: int, device, rank: int, world: int, fmt: int = 0,
                 sync: bool = False, gather=None, keep_capture: bool = False, parity_samples: int = 0, checks: bool = True,
                 keep_last: bool = False):
    import torch
    import torch.distributed as dist
    from snout_amd.rx import SnoutRx
    proto, n_ch, channel, _, _, descr = WORKLOADS[name]
    tiles, truths = make_tiles(name, 2 + rank, device)
    x = resident_capture(tiles, n, seed=2 + rank, device=device)
    expect = expected_ok(name, truths, tiles.shape[1] // 2, n)
    pdus = {p.payload for tr in truths for p in tr}
    del tiles
    if fmt:
        x = quantise(x, fmt)
        torch.cuda.empty_cache()
    # with a GPU exchange attached the records stay in device memory: the exchange packs them from there
    on_dev = gather is not None and gather.on_gpu
    rcus = reserved_cus(world, gather.fake if gather is not None else 0) if n_ch > 1 else 0
    rx = SnoutRx(proto=proto, channel=channel, n_channels=n_ch, device=device.index, sample_format=fmt, records_on_device=on_dev,
                 reserved_cus=rcus, zb_core=int(os.environ.get("SNOUT_BENCH_ZB_CORE", "0")),
                 zb_warmup=int(os.environ.get("SNOUT_BENCH_ZB_WARMUP", "0")))        # dev aid: 802.15.4 lane shape (0 = the default rule)

    gathered = [0, 0]                   # exchanges finished on rank 0, records in the last one
    held = [None]                       # rank 0's views of the last exchange (keep_last: copied after the timed steps)

    def take_exchange():
        parts = gather.finish(views=True)
        if parts is not None:
            gathered[0] += 1
            gathered[1] = int(sum(len(v) for v in parts))
            held[0] = parts

    def finish_one():
        pk = rx.collect(copy=False)                             # a count when the records stay on the device
        if gather is not None:
            # RCCL gather of this step's records to rank 0, overlapped with the next step
            if len(gather.inflight) == 2:
                take_exchange()
            gather.begin(int(pk if on_dev else pk.size))
            gather.append(pk, rx=rx)                            # packed from the device copy by one kernel: no upload
            gather.launch()
        return pk

    def run_steps(k):
        last = None
        if sync:
            for _ in range(k):
                rx.submit(x, first_sample_index=rank * n)
                last = finish_one()
            return last
        for i in range(k):
            if gather is not None:
                gather.sync_uploads()       # result slots about to be reused have been read
            rx.submit(x, first_sample_index=rank * n)
            if i >= 2:                      # two segments stay queued behind the one being collected
                last = finish_one()
        for _ in range(min(k, 2)):
            last = finish_one()
        return last

    def fence():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(device)

    def drain():
        while gather is not None and gather.inflight:
            take_exchange()

    # prime the pipeline: first-use allocations of the result slots and the HIP runtime's own
    # lazily grown pools (two ~7 ms stalls were measured around the 11th and 16th submit of a process)
    run_steps(24 if n <= int(1.1e9) else 8)
    if warmup:
        run_steps(warmup)
    drain()
    fence()
    # the interpreter's cyclic collector stays out of the timed steps (a generation-2 pass is several ms of host time: two of
    # the three queued steps' worth)
    gc.collect()
    gc.disable()
    t0 = time.perf_counter()
    last = run_steps(steps)
    drain()                 # every step's records are on rank 0 before the clock stops
    fence()
    dt = time.perf_counter() - t0
    gc.enable()
    # keep_last: the records the caller got from the last timed step (rank 0's gathered ones with an exchange attached),
    # copied before the next submit or exchange reuses the buffers behind them
    last_records = None
    if keep_last:
        last_records = owned_records([last]) if gather is None else (owned_records(held[0]) if held[0] is not None else None)
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    k_ms = rx.profile_history()[-min(steps, 64):]

    # correctness of the timed work: every generated packet decoded with a good CRC
    local = rx.process(x, first_sample_index=rank * n)
    n_ok = int(local["crc_ok"].sum())
    fcs = 3 if proto == 0 else 0        # BTLE records carry PDU + CRC24, truth holds the PDU; 802.15.4: PSDU incl. FCS
    seen = {bytes(p["bytes"][:p["len"] - fcs]) for p in local[:4096] if p["crc_ok"]}
    assert n_ok >= expect, f"{name} rank {rank}: decoded {n_ok} CRC-ok packets, expected >= {expect}"
    assert seen <= pdus, "decoded a PDU that was never transmitted"
    prof = rx.profile()
    k_avg = float(np.mean(k_ms))
    if proto == 1 and n_ch == 1 and not sync:
        # the 802.15.4 chain is several kernels on two streams: pipelined, its event pair also spans
        # the overlap with the neighbouring steps, so its duration comes from one-at-a-time passes
        ks = []
        for _ in range(3):
            rx.process(x, first_sample_index=rank * n, copy=False)
            ks.append(rx.profile().ms_dominant)
        k_avg = float(np.mean(ks))
    algo = float(x.element_size() * 2) * n + 160.0 * len(local)
    res = {"workload": "%s, %.3g %s samples per GPU resident in HBM" % (descr, n, ["cf32", "sc8", "sc16"][fmt]),
           "value": n * world * steps / dt / 1e6, "unit": "Msamples/s", "ms_per_step": dt / steps * 1e3,
           "steps": steps, "samples_per_gpu": n, "packets_per_gpu": int(len(local)),
           "decoded_pkts_per_s": len(local) * world * steps / dt,
           "decoded_crc_ok_per_gpu": n_ok, "min_expected_crc_ok_per_gpu": expect,
           "kernel": prof.dominant_name, "kernel_ms": k_avg, "algorithmic_bytes": algo,
           "achieved_GBps": algo / (k_avg * 1e-3) / 1e9, "frac": algo / (k_avg * 1e-3) / 1e9 / HBM_PEAK_GBPS,
           # `frac` prices the DOMINANT KERNEL's HIP-event duration; `step_frac` the whole step (kernels + compaction + record
           # D2H: SURVEY 8d's timed region) on the same algorithmic bytes
           "step_frac": algo / (dt / steps) / 1e9 / HBM_PEAK_GBPS}
    if n_ch > 1:
        fl = PFB_FLOP[n_ch] * n
        res["fp32"] = {"flop_per_sample": float(PFB_FLOP[n_ch]), "achieved_TFLOPs": fl / (k_avg * 1e-3) / 1e12,
                       "peak_TFLOPs": FP32_PEAK_TFLOPS, "frac": fl / (k_avg * 1e-3) / 1e12 / FP32_PEAK_TFLOPS}
    if gather is not None:
        # the last timed step's exchange as rank 0 received it: every rank's records of that step
        how = " all_gather (32-B headers) + gather to rank 0 (records)" if gather.to_root else " all_gather_into_tensor"
        res["collective"] = ("RCCL" + how) if gather.backend == "nccl" else (
            gather.backend + how if gather.collective else "none (device copy)")
        res["ranks_in_collective"] = gather.world
        res["records_on_rank0_last_step"] = gathered[1]
        # every rank's records of the last timed step arrived: the exchange is deterministic, so the count rank 0 holds
        # must EQUAL the sum of what the ranks decode from their captures (x the blocks of a fake-world rehearsal)
        total = torch.tensor([len(local)], dtype=torch.int64, device=device if gather.backend == "nccl" else "cpu")
        if world > 1:
            dist.all_reduce(total, group=gather.group)
        if rank == 0:
            assert gathered[0] == (24 if n <= int(1.1e9) else 8) + warmup + steps, gathered
            assert gathered[1] == int(total.item()) * (gather.fake or 1), (gathered, int(total.item()))
        if gather.fake:
            res["fake_world"] = gather.fake
        res["reserved_cus"] = rcus
    if last_records is not None:
        res["last_records"] = last_records
    rx.close()
    if parity_samples:
        # the whole capture where the oracle finishes it in seconds (first_sample_index 0: rank 0's own capture)
        full = parity_samples >= n and rank == 0
        res["parity_in_run"] = parity_in_run(x, name, min(parity_samples, n), device, fmt, got=local if full else None)
    if checks and proto == 1 and rank == 0 and not os.environ.get("SNOUT_BENCH_ZB_CORE"):
        # what the default (timed) decode loses against the reference's one sequential loop
        # (the prefix spans every distinct tile of the capture: 32 x 2^21 / 32 x 2^19 samples)
        shapes = FIDELITY_SHAPES if world == 1 else ()
        fl = lost_vs_sequential(x, name, min(n, (1 << 26) if n_ch > 1 else (1 << 24)), device, fmt, shapes=shapes)
        for core, warm in shapes:
            # what that fidelity costs: the same pipelined steps on the same capture with the longer lanes
            with SnoutRx(proto=proto, channel=channel, n_channels=n_ch, device=device.index, sample_format=fmt, zb_core=core, zb_warmup=warm) as r2:
                def loop(m):
                    for i in range(m):
                        r2.submit(x, first_sample_index=rank * n)
                        if i >= 2:
                            r2.collect(copy=False)
                    for _ in range(min(m, 2)):
                        r2.collect(copy=False)
                loop(8)
                torch.cuda.synchronize(device)
                t1 = time.perf_counter()
                loop(10)
                torch.cuda.synchronize(device)
                fl["fidelity_modes"]["%d / %d" % (core, warm)]["ms_per_step"] = (time.perf_counter() - t1) / 10 * 1e3
        if shapes:
            fl["fidelity_modes"]["%s (default)" % ("6144 / 3072" if n_ch > 1 else "6144 / 1024")] = {"lost": fl["lost"], "extra": fl["extra"], "frac_lost": fl["frac_lost"],
                                                             "frac_extra": fl["frac_extra"], "ms_per_step": res["ms_per_step"]}
        res["frames_lost_vs_sequential"] = fl
    if keep_capture:
        return res, x
    del x
    torch.cuda.empty_cache()
    return res, None


def read_peak(x, device):
    """Read-only streaming rate of the resident capture, measured in this process (GB/s)."""
    import torch
    from snout_amd import _ffi
    lib = _ffi.load()
    best, mean = C.c_float(0), C.c_float(0)
    nbytes = min(x.numel() * x.element_size(), 8 << 30)
    st = torch.cuda.current_stream(device).cuda_stream
    _ffi.check(lib.snout_bench_hbm_read_gbps(C.c_void_p(x.data_ptr()), nbytes, 10, C.c_void_p(st),
                                       C.byref(best), C.byref(mean)))
    return float(best.value), float(mean.value)


def traffic_from_profiles(workload: str, kernel: str, n: int):
    """PMC-derived HBM bytes per launch of the same kernel / workload, from the committed profile
    pass (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, gfx950-corrected); None when there is none."""
    for name in ("r6_traffic.json", "r5_traffic.json", "r4_traffic.json", "r3_traffic.json", "r2_traffic.json", "r1_traffic.json"):
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        tj = json.load(open(path))
        for e in (tj if isinstance(tj, list) else [tj]):
            if e.get("workload") == workload and e.get("workload_samples") == n and e.get("kernel") == kernel:
                return e["traffic_bytes_per_launch"], "profiles/" + name
            if "workload" not in e and workload == "cfg2" and e.get("workload_samples") == n and e.get("kernel") == kernel:
                return e["traffic_bytes_per_launch"], "profiles/" + name
    return None, None


# ------------------------------------------------------------------------------------------------
# cfg #5: both wideband scans concurrently, sharded in 2^24-sample segments
# ------------------------------------------------------------------------------------------------
def run_cfg5(steps: int, warmup: int, device, rank: int, world: int, seconds: float = 10.0, group=None, parity: bool = False,
             keep_last: bool = False):
    import torch
    import torch.distributed as dist
    from snout_amd import dist as sdist
    from snout_amd.sharded import ShardedScan
    nb_rank, nz_rank = int(80e6 * seconds), int(32e6 * seconds)
    on_gpu = (not dist.is_initialized()) or dist.get_backend(group) == "nccl"
    # Every rank's segments of one step go to the library as ONE submission per scan (snout_rx_submit_batch_dev: up to 64
    # segments run side by side in the same launches -- 48 segments of 2^24 samples at the rate of one 8e8-sample segment),
    # the records stay in device memory (the exchange packs them from there) and the scans never drain between two steps.
    fake = int(os.environ.get("SNOUT_BENCH_FAKE_WORLD", "0")) if world == 1 else 0
    reserved = reserved_cus(world, fake)
    sb = ShardedScan(0, n_channels=40, seg_len=SEG, device=device.index, handles=int(os.environ.get("SNOUT_CFG5_HB", "1")),
                     batch=int(os.environ.get("SNOUT_CFG5_BB", "48")), depth=3, records_on_device=on_gpu, reserved_cus=reserved,
                     stream_priority=int(os.environ.get("SNOUT_CFG5_BPRIO", "0")))
    sz = ShardedScan(1, n_channels=16, seg_len=SEG, device=device.index, handles=int(os.environ.get("SNOUT_CFG5_HZ", "1")),
                     batch=int(os.environ.get("SNOUT_CFG5_BZ", "20")), depth=3, records_on_device=on_gpu, reserved_cus=reserved,
                     zb_core=int(os.environ.get("SNOUT_CFG5_ZB_CORE", "0")), zb_warmup=int(os.environ.get("SNOUT_CFG5_ZB_WARMUP", "0")),
                     stream_priority=int(os.environ.get("SNOUT_CFG5_ZPRIO", "-1")))
    # The virtual capture is N x `seconds` long; its tile g (a sixth / an eighth of a segment) is tile g mod TILES of
    # TILES independently seeded tiles of traffic -- the same on every rank, so the overlap a rank reads behind its segment
    # i shows the packets the next rank finds at the start of segment i + 1 (only the noise differs) and the duplicates
    # meet in rank 0's de-duplication.  Each rank keeps ITS segments in HBM, one block of seg_len + overlap + pre-roll
    # samples per segment (local segment j = global segment rank + j N), every block with its own noise.
    tiles_b, truths_b = make_tiles("cfg3", 3, device, n_tile=sb.seg_len // 6)
    tiles_z, truths_z = make_tiles("cfg4", 4, device, n_tile=sz.seg_len // 8)
    Lb, Lz = tiles_b.shape[1] // 2, tiles_z.shape[1] // 2
    assert sb.seg_len % Lb == 0 and sz.seg_len % Lz == 0
    caps = []
    for sc, tiles, n_rank, seed in ((sb, tiles_b, nb_rank, 3), (sz, tiles_z, nz_rank, 4)):
        n_total = n_rank * world
        segs = sdist.shard_segments(n_total, sc.seg_len, sc.overlap, rank, world, sc.preroll, uniform=True)
        S, pre, P = sc.seg_len, sc.preroll, sc.pad_to
        x = torch.zeros(2 * len(segs) * P, dtype=torch.float32, device=device)
        g = torch.Generator(device=device)
        g.manual_seed(1000 + seed + 10 * rank)
        for j, (a, b) in enumerate(segs):
            fill_capture(x[2 * j * P:2 * (j * P + (b - a))], a, tiles, g)
        torch.cuda.synchronize(device)

        def source(a, b, x=x, S=S, pre=pre, P=P):
            j = ((a + pre) // S) // world           # a = max(0, i S - preroll) of global segment i = rank + j N
            return x[2 * j * P:2 * (j * P + (b - a))]
        caps.append((n_total, source, x))
    del tiles_b, tiles_z
    (nb, srcb, xb), (nz, srcz, xz) = caps
    gdev = device if on_gpu else None
    # 96-byte BTLE wire records: 24 + (2 + 63 + 3), the longest PDU the decoder can emit (a false access-address match on
    # a data channel carries a 6-bit length).  The capacity is the same number on every rank (no collective to agree it).
    hint_b, hint_z = nb_rank // 8000, nz_rank // 8000
    gb = sdist.AsyncRecordGather(gdev, group, width=96, dedup_tol=0, cap=hint_b + hint_b // 4 + 1024, fake_world=fake, prealloc=6)
    gz = sdist.AsyncRecordGather(gdev, group, width=160, dedup_tol=8 * 64 + 8, cap=hint_z + hint_z // 4 + 1024, fake_world=fake, prealloc=6)
    results = {"b": None, "z": None}
    trace = [] if os.environ.get("SNOUT_BENCH_TRACE") else None     # dev aid: where the host thread's time goes
    sb.trace = sz.trace = trace
    closed = {"b": 0, "z": 0}
    launched = [0]

    def on_last(g, key):
        g.close()
        closed[key] += 1

    def queue_step():
        sb.start(nb, srcb, group, sink=gb, on_first=gb.begin, on_last=lambda: on_last(gb, "b"))
        sz.start(nz, srcz, group, sink=gz, on_first=gz.begin, on_last=lambda: on_last(gz, "z"))

    def pump_until(pred):
        """Drive both scans from this one host thread until pred(): each submits while it has a free slot and collects
        what has finished; the thread waits (in one scan's collect) only when neither can do either."""
        while not pred():
            live = [sc for sc in (sb, sz) if sc.active()]
            if not any([sc.step(block=False) for sc in live]):
                live[0].step()

    def take():
        b, z = gb.finish(views=True), gz.finish(views=True)      # zero-copy views of rank 0's pinned buffers
        if rank == 0:
            results["b"], results["z"] = b[0], z[0]

    def launch_next():
        """The exchanges of the oldest complete step, in the same order on every rank (the two gathers share the process
        group).  Two exchanges of each are in flight: the exchange of step i overlaps the kernels of step i + 1."""
        k = launched[0] + 1
        pump_until(lambda: closed["b"] >= k and closed["z"] >= k)
        t_a = time.perf_counter()
        if len(gb.inflight) == 2:
            take()
        t_b = time.perf_counter()
        gb.launch()
        gz.launch()
        launched[0] = k
        if trace is not None:
            trace.append(("take", t_b - t_a))
            trace.append(("launch exchanges", time.perf_counter() - t_b))

    def run_steps(k):
        base = launched[0]
        ahead = int(os.environ.get("SNOUT_CFG5_AHEAD", "2"))
        for i in range(k):
            queue_step()                            # step i's submissions are queued behind step i - 1's: no drain between
            if i >= ahead:
                # step i - ahead complete on both scans -> its exchanges.  Two steps stay queued behind the one being
                # finished (round 5): with one, the scan that finishes its step first (BTLE) had nothing queued while the host
                # waited for the other's (802.15.4: clock recovery + sinks + frame repair) -- 2-3 ms of idle channelizer per step
                launch_next()
        while launched[0] < base + k:
            launch_next()
        while gb.inflight:                          # every step's records are on rank 0, de-duplicated
            take()

    def fence():
        torch.cuda.synchronize(device)
        if world > 1:
            dist.barrier(group)
        torch.cuda.synchronize(device)

    # every (handle, work set, result slot) combination has to have carried the step's large batch once before the clock
    # starts -- their buffers grow on first use (GBs of hipMalloc for a 20-segment 802.15.4 batch): six steps cover the
    # rotation of 2 handles x 2 work sets x 3 submissions per step
    run_steps(max(6, warmup))
    fence()
    if trace is not None:
        del trace[:]
    gc.collect()
    gc.disable()
    t0 = time.perf_counter()
    run_steps(steps)
    fence()
    dt = time.perf_counter() - t0
    gc.enable()
    # keep_last: rank 0's de-duplicated records of the last timed step, copied out of the exchanges' pinned buffers
    last_records = {"btle": owned_records([results["b"]]), "zigbee": owned_records([results["z"]])} if keep_last and rank == 0 else None
    if trace is not None and rank == 0:
        import collections
        agg, cnt = collections.Counter(), collections.Counter()
        for what, sec in trace:
            agg[what] += sec
            cnt[what] += 1
        print("host trace over warm-up + %d steps (%.1f ms wall in the timed steps):" % (steps, dt * 1e3), file=sys.stderr)
        for what, sec in agg.most_common():
            print("  %-28s %5d calls %9.2f ms  (%.3f ms each)" % (what, cnt[what], sec * 1e3, sec * 1e3 / cnt[what]), file=sys.stderr)
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=device if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX, group=group)
        dt = float(tmax.item())
    # what the record exchange ran on, and how many ranks one all_gather of rank ids actually reached
    if dist.is_initialized():
        ids = torch.full((1,), rank, dtype=torch.int64, device=device if dist.get_backend(group) == "nccl" else "cpu")
        seen = torch.empty(dist.get_world_size(group), dtype=torch.int64, device=ids.device)
        dist.all_gather_into_tensor(seen, ids, group=group)
        assert sorted(seen.tolist()) == list(range(dist.get_world_size(group)))
        bk = "RCCL" if dist.get_backend(group) == "nccl" else dist.get_backend(group)
        collective = bk + (" all_gather (32-B headers) + gather to rank 0 (records)" if gb.to_root else " all_gather_into_tensor")
        n_seen = int(seen.numel())
    else:
        collective, n_seen = "none (no process group: device copy)", 1
    want_recs, t_oracle = None, 0.0
    if parity and not fake:
        # cfg #5 against the oracle AS cfg #5, at every world size: every rank decodes ITS
        # segments with the CPU oracle (same cuts, overlaps, pre-roll, padding, lane shape; what lies before a segment's own
        # range dropped as the scan drops it), the records travel to rank 0 by dist.gather_records, and rank 0 compares the
        # host statement of the de-duplication rule over them with what the GPU path delivered for the last timed step:
        # every field and byte; outside the timed region.  What the consumer keeps: snout/core/message.py:226 (CRC0 lines),
        # snout/util/zigbee.py:194-202 (every PDU).
        from oracle import oracle_py
        t_or = time.perf_counter()
        oracle_py.set_threads(max(1, oracle_py.hw_threads() // world))
        try:
            want_recs = {}
            for name, sc, src in (("btle", sb, srcb), ("zigbee", sz, srcz)):
                parts = [np.zeros(0, dtype=_pkt_dtype())]
                for j, (a, b) in enumerate(sc._segs):
                    host = src(a, b).cpu().numpy()
                    if (b - a) < sc.pad_to:             # the capture's last segment, padded to the batch's length as the scan pads it
                        host = np.concatenate([host, np.zeros(2 * (sc.pad_to - (b - a)), dtype=host.dtype)])
                    rec = oracle_py.wideband_segment(host, proto=sc.proto, first_sample_index=a // sc.decim)
                    g_seg = rank + j * world
                    own = (g_seg * sc.seg_len) // sc.decim if (g_seg and sc.preroll) else 0
                    parts.append(rec[rec["sample_index"] >= own] if own else rec)
                mine = np.concatenate(parts)
                want_recs[name] = sdist.gather_records(mine, device if on_gpu else None, group) if world > 1 else mine
        finally:
            oracle_py.set_threads(1)
        t_oracle = time.perf_counter() - t_or
        if rank != 0:
            want_recs = None
    res = None
    if rank == 0:
        rb, rz = results["b"], results["z"]
        ok_b, ok_z = int(rb["crc_ok"].sum()), int(rz["crc_ok"].sum())
        mult = fake or 1
        exp_b = int(0.9 * truth_in(truths_b, Lb, nb)) * mult
        exp_z = int(0.8 * truth_in(truths_z, Lz, nz)) * mult
        assert ok_b >= exp_b and ok_z >= exp_z, (ok_b, exp_b, ok_z, exp_z)
        key = (rb["channel"].astype(np.uint64) << np.uint64(48)) | rb["sample_index"]
        assert np.all(key[1:] > key[:-1]), "BTLE records on rank 0 are not sorted / de-duplicated"
        fcs_ok = {bytes(p["bytes"][:p["len"] - 3]) for p in rb[:2048] if p["crc_ok"]}
        assert fcs_ok <= {p.payload for tr in truths_b for p in tr}, "decoded a PDU that was never transmitted"
        total = (nb + nz) * steps
        res = {"workload": CFG5_DESCR, "value": total / dt / 1e6, "unit": "Msamples/s",
               "ms_per_step": dt / steps * 1e3, "steps": steps,
               "samples_per_gpu": nb_rank + nz_rank, "btle_samples_per_gpu": nb_rank, "zigbee_samples_per_gpu": nz_rank,
               "segments_per_gpu": len(sb._segs) + len(sz._segs), "segment_samples": SEG,
               "segments_per_submission": {"btle": sb.batch, "zigbee": sz.batch}, "reserved_cus": reserved,
               "value_per_gpu": total / dt / 1e6 / world, "collective": collective, "ranks_in_collective": n_seen,
               "device_of_rank0": int(device.index),
               "records_on_rank0": int(len(rb) + len(rz)), "decoded_crc_ok": ok_b + ok_z,
               "min_expected_crc_ok": exp_b + exp_z, "decoded_pkts_per_s": (len(rb) + len(rz)) / mult * steps / dt,
               "sharding": "segment i -> rank i mod N; per step one exchange of 96-B BTLE and one of 160-B "
                           "802.15.4 records to rank 0 (%s), sort + de-duplication on rank 0's GPU, inside the "
                           "timed region" % (collective if dist.is_initialized() else "single rank: device copy"),
               "algorithmic_bytes": 8.0 * (nb_rank + nz_rank) + 160.0 * (len(rb) + len(rz)) / mult / world}
        if fake:
            res["fake_world"] = {"blocks_on_rank0": fake, "note": "rehearsal at world size 1: rank 0 sorts, de-duplicates and downloads "
                                 "%d copies of its own records per step (sample_index shifted per copy), as it will at N = %d" % (fake, fake)}
        if last_records is not None:
            res["last_records"] = last_records
        res["achieved_GBps"] = res["algorithmic_bytes"] / (res["ms_per_step"] * 1e-3) / 1e9
        res["frac"] = res["step_frac"] = res["achieved_GBps"] / HBM_PEAK_GBPS       # (priced on the whole step)
        if want_recs is not None:
            res["parity_in_run"] = {}
            for name, sc, got, tol in (("btle", sb, rb, 0), ("zigbee", sz, rz, 8 * 64 + 8)):
                want = sdist.dedup_records(want_recs[name], tol=tol)
                have = sdist.widen_records(np.asarray(got))
                equal = len(want) == len(have) and all(np.array_equal(want[f], have[f]) for f in PARITY_FIELDS) \
                    and np.array_equal(want["bytes"], have["bytes"])
                assert equal, f"cfg5 {name}: rank 0's records of one step differ from the oracle's ({len(have)} vs {len(want)})"
                res["parity_in_run"][name] = {"segments_per_rank": len(sc._segs), "records": int(len(want)),
                                              "crc_ok_records": int(want["crc_ok"].sum()), "equal": True}
            res["parity_in_run"]["oracle_s"] = round(t_oracle, 2)
            res["parity_in_run"]["ranks"] = world
            res["parity_in_run"]["compared"] = ("rank 0's sorted, de-duplicated records of the last timed step (every rank's segments, gathered) against "
                                                "the CPU oracle run by every rank on ITS segments, gathered (dist.gather_records) + "
                                                "dist.dedup_records: every record field and byte")
            if world == 1:
                # the 802.15.4 scan's traffic is cfg #4's: what the timed (default) decode loses against one sequential lane
                # (a prefix that spans every distinct tile)
                res["frames_lost_vs_sequential"] = lost_vs_sequential(xz, "cfg4", min(1 << 26, xz.numel() // 2), device, 0)
    sb.close()
    sz.close()
    del xb, xz, caps
    torch.cuda.empty_cache()
    return res


CFG5_FIELDS = ("workload", "value", "unit", "ms_per_step", "steps", "segments_per_gpu", "segments_per_submission", "records_on_rank0",
               "decoded_crc_ok", "min_expected_crc_ok", "frac", "step_frac", "value_per_gpu", "collective", "ranks_in_collective", "achieved_GBps",
               "sharding", "fake_world", "reserved_cus", "parity_in_run", "frames_lost_vs_sequential")


# ------------------------------------------------------------------------------------------------
def visible_gpus(sysfs: str = "/sys/class/kfd/kfd/topology/nodes"):
    """GPUs a child process would see, counted WITHOUT the HIP / HSA runtime (torch.cuda.device_count()
    falls back to hipGetDeviceCount on ROCm, which opens KFD in a process whose only job is to start the ranks): the KFD
    topology nodes with simd_count > 0, narrowed by a non-empty ROCR_ / HIP_ / CUDA_VISIBLE_DEVICES list.  None when the
    topology is not readable (then the ranks themselves fail fast)."""
    try:
        nodes = sorted(os.listdir(sysfs), key=lambda s: int(s) if s.isdigit() else 1 << 30)
    except OSError:
        return None
    have = 0
    for node in nodes:
        try:
            props = dict(ln.split()[:2] for ln in open(os.path.join(sysfs, node, "properties")) if len(ln.split()) >= 2)
        except OSError:
            continue                            # a node this user may not read is not a GPU it may use
        if int(props.get("simd_count", "0")) > 0:
            have += 1
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        val = os.environ.get(var, "").strip()
        if val:                                 # an index (or UUID) list: entries beyond the topology do not count
            ids = [v.strip() for v in val.split(",") if v.strip()]
            have = min(have, sum(1 for v in ids if not v.lstrip("-").isdigit() or 0 <= int(v) < have))
    return have


def self_launch(n: int) -> int:
    """Start `python -m torch.distributed.run --nnodes=1 --nproc-per-node n bench.py <same arguments>` as a child process,
    stream its output, print rank 0's JSON line as the one and last JSON line of stdout.  Returns the child's exit code."""
    import subprocess
    backend = os.environ.get("SNOUT_BENCH_BACKEND", "nccl")
    if backend == "nccl":
        have = visible_gpus()                   # from sysfs: this process never opens the HIP runtime (it only starts children)
        if have is not None and have < n:
            print(f"bench.py --gpus {n}: {have} GPU(s) visible; one rank per GPU needs {n} "
                  "(SNOUT_BENCH_BACKEND=gloo shares devices between ranks: a debugging aid, not a measurement)", file=sys.stderr)
            return 2
    # --standalone: the launcher's own c10d rendezvous on a port IT picks (no bind / close / reuse race of ours)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           "--nproc-per-node", str(n), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    last_json = None
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True, bufsize=1)
    for line in proc.stdout:
        if line.startswith("{") and '"metric"' in line:
            last_json = line                    # held back: printed once, as the last line
            continue
        sys.stdout.write(line)
        sys.stdout.flush()
    rc = proc.wait()
    if last_json is not None:
        sys.stdout.write(last_json if last_json.endswith("\n") else last_json + "\n")    # the contract: ONE JSON line, last on stdout
        sys.stdout.flush()
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["cfg5"], default=None,
                    help="run this workload alone (default: cfg3 at every N, the others in other_workloads: all at N = 1, cfg5 at N > 1)")
    ap.add_argument("--samples", type=float, default=0,
                    help="complex input samples per GPU per step (default: the workload's BASELINE size)")
    ap.add_argument("--seconds", type=float, default=10.0, help="cfg5: seconds of each band per GPU")
    ap.add_argument("--format", choices=["cf32", "sc8", "sc16"], default="cf32",
                    help="input sample format resident in HBM (cf32 is BASELINE's; sc8 = HackRF / upstream "
                         "btle_rx int8 IQ, sc16 = USRP): the same capture quantised on the device")
    ap.add_argument("--cpu-samples", type=float, default=0,
                    help="samples of the CPU baseline legs (default: ~10 s of oracle time per leg)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--parity", choices=["full", "prefix"], default="full",
                    help="parity_in_run of cfg2 / cfg3 / cfg4: the whole capture against the oracle (default; tens of seconds of "
                         "host time outside the timed region) or only the CPU leg's prefix")
    ap.add_argument("--no-others", action="store_true", help="N = 1: skip the other_workloads block")
    ap.add_argument("--sync", action="store_true",
                    help="one segment at a time (no submit/collect pipelining); for profiling")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the records of the last timed step (rank 0) as DIR/<name>_<field>.npy, float32 / float64, "
                         "at most 64 MB in all (a fixed seeded sample of the rows beyond that)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself (what replaces the sequential hop of
        # snout/core/radio.py:415): this process has touched no GPU, so it starts the N ranks as a CHILD (never an exec),
        # passes their output through, prints rank 0's JSON once more as ITS last line of stdout and exits with their code
        sys.exit(self_launch(args.gpus))

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch `python bench.py --gpus N` by itself, or "
                         "torch.distributed.run --nproc-per-node N bench.py --gpus N")
    # one rank per GPU; SNOUT_BENCH_BACKEND=gloo lets the multi-rank code path be exercised on a box
    # with fewer GPUs than ranks (ranks then share devices; a debugging aid, not a measurement)
    backend = os.environ.get("SNOUT_BENCH_BACKEND", "nccl")
    local_rank = local_rank % max(1, torch.cuda.device_count()) if backend != "nccl" else local_rank
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    assert torch.cuda.current_device() == local_rank            # LOCAL_RANK -> device
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # the record exchange is a few MB per step: a few RCCL channels carry it, and every channel is a workgroup that
        # needs a CU beside the channelizer's persistent grid (which leaves reserved_cus free for them)
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "8")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    elif os.environ.get("SNOUT_BENCH_NCCL1") == "1":
        # a one-GPU box: the record exchange of cfg #5 still runs as a real RCCL collective (world size 1), so the
        # path an 8-GPU run takes (all_gather_into_tensor on device buffers, device dedup, pack_last_records) executes
        import socket
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=device)

    from snout_amd import dist as sdist
    fmt = {"cf32": 0, "sc8": 1, "sc16": 2}[args.format]
    # The same workload at every N (weak scaling: every rank its own capture segment of the BASELINE size, the decoded
    # records gathered to rank 0 over RCCL inside the timed region), so that value(N) / (N value(1)) is a scaling
    # efficiency.  BASELINE.json configs[4] (both scans in 2^24-sample segments dealt over the ranks) rides along as
    # other_workloads.cfg5 at every N and is the headline with --workload cfg5.
    headline = args.workload or "cfg3"
    out = None
    dump = {}                                   # --dump-outputs: name -> the last timed step's records (rank 0)

    def cfg5_run(steps, warmup, parity, keep_last=False):
        """cfg #5 with its parity_in_run: on the timed capture itself at N = 1; at N > 1 on a separate pass over 1 s of each
        band per rank (N ranks share the host's cores: the oracle on N x 10 s would take minutes)."""
        full = world == 1 or args.seconds <= 1.0
        r5 = run_cfg5(steps, warmup, device, rank, world, seconds=args.seconds, parity=parity and full, keep_last=keep_last)
        if parity and not full:
            rp = run_cfg5(2, 1, device, rank, world, seconds=1.0, parity=True)
            if rank == 0:
                r5["parity_in_run"] = dict(rp["parity_in_run"], capture="a separate pass: 1 s of each band per rank, 2 steps")
        return r5

    if headline == "cfg5":
        r5 = cfg5_run(args.steps, args.warmup, not args.no_cpu, keep_last=args.dump_outputs is not None)
        if rank == 0:
            dump = {k + "_records": v for k, v in r5.pop("last_records", {}).items()}
            out = {"metric": METRIC, "value": r5["value"], "unit": "Msamples/s", "n_gpus": world,
                   "steps": args.steps, "warmup": args.warmup, "ms_per_step": r5["ms_per_step"],
                   "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
                   "data": "synthetic", "config": {k: r5[k] for k in r5 if k not in ("value", "unit", "ms_per_step", "steps")},
                   "roofline": {"bound": "hbm", "achieved": r5["achieved_GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                                "frac": r5["frac"], "traffic": None, "kernel": "whole step (pfb_channelize<40>, "
                                "pfb_channelize<16> and the 802.15.4 chain on small segments)",
                                "kernel_ms": r5["ms_per_step"], "algorithmic_bytes": r5["algorithmic_bytes"],
                                "note": "per-GPU algorithmic bytes over the whole step: small segments are "
                                        "launch-bound, see the single-segment kernels' fractions at N = 1"}}
    else:
        n = int(args.samples or WORKLOADS[headline][3])
        # N > 1: the per-step record gather; SNOUT_BENCH_NCCL1=1 on a one-GPU box runs the same exchange on RCCL at world 1
        fake = int(os.environ.get("SNOUT_BENCH_FAKE_WORLD", "0")) if world == 1 else 0
        gather = (sdist.AsyncRecordGather(device, width=WORKLOADS[headline][4], fake_world=fake)
                  if (world > 1 or dist.is_initialized() or fake > 1) else None)
        res, x = run_workload(headline, n, args.steps, args.warmup, device, rank, world, fmt=fmt, sync=args.sync,
                              gather=gather, keep_capture=True, checks=not args.no_cpu,       # (--no-cpu: profiling runs, no checks)
                              keep_last=args.dump_outputs is not None)
        if "last_records" in res:
            dump = {"records": res.pop("last_records")}
        if rank == 0:
            traffic, tsrc = (traffic_from_profiles(headline, res["kernel"], n) if fmt == 0 else (None, None))
            rbest, rmean = read_peak(x, device)
            roof = {"bound": "hbm", "achieved": res["achieved_GBps"], "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": res["frac"], "traffic": traffic, "traffic_source": tsrc,
                    "kernel": res["kernel"], "kernel_ms": res["kernel_ms"], "algorithmic_bytes": res["algorithmic_bytes"],
                    "step_frac": res["step_frac"], "measured_read_GBps": rbest, "measured_read_mean_GBps": rmean,
                    "frac_of_measured_read": res["achieved_GBps"] / rbest if rbest else None}
            if "fp32" in res:
                roof["fp32"] = res["fp32"]
                roof["fp32_frac"] = res["fp32"]["frac"]
                roof["fp32_achieved_TFLOPs"] = res["fp32"]["achieved_TFLOPs"]
            out = {"metric": METRIC, "value": res["value"], "unit": "Msamples/s", "n_gpus": world,
                   "steps": args.steps, "warmup": args.warmup, "ms_per_step": res["ms_per_step"],
                   "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                   "dtype": "f32" if fmt == 0 else ("i8->i32" if (fmt == 1 and headline == "cfg2") else args.format + "->f32"),
                   "data": "synthetic",
                   "config": {"workload": res["workload"], "samples_per_gpu": n, "packets_per_gpu": res["packets_per_gpu"],
                              "decoded_pkts_per_s": res["decoded_pkts_per_s"],
                              "sharding": ("every rank its own segment, per-step %s gather of %d-B records to rank 0"
                                           % (gather.backend, WORKLOADS[headline][4])) if gather is not None else "single segment",
                              **({k: res[k] for k in ("collective", "ranks_in_collective", "records_on_rank0_last_step", "fake_world", "reserved_cus") if k in res}
                                 if gather is not None else {}),
                              "decoded_crc_ok_per_gpu": res["decoded_crc_ok_per_gpu"],
                              "min_expected_crc_ok_per_gpu": res["min_expected_crc_ok_per_gpu"],
                              "stepping": "one segment at a time" if args.sync else
                                          "pipelined: record D2H of step i overlaps step i+1"},
                   "roofline": roof}
            if "frames_lost_vs_sequential" in res:
                out["config"]["frames_lost_vs_sequential"] = res["frames_lost_vs_sequential"]
            if not args.no_cpu and world == 1:      # the CPU baseline is timed at N = 1 only
                ns = int(min(args.cpu_samples or CPU_SAMPLES[headline], n))
                out["cpu_baseline"], cpu_recs = cpu_baseline(x, headline, ns)
                # the records the one-thread CPU leg just produced against the HIP path on the same samples ...
                out["parity_in_run"] = parity_in_run(x, headline, ns, device, fmt, want=cpu_recs)
                if headline in PARITY_FULL and args.parity != "prefix" and ns < n:
                    # ... and the WHOLE capture: the oracle as one segment on every host thread, outside the timed region
                    out["parity_in_run"] = dict(parity_in_run(x, headline, n, device, fmt), cpu_leg_prefix=out["parity_in_run"])
        del x
        torch.cuda.empty_cache()
        if world == 1 and args.workload is None and not args.no_others:
            others = {}
            k = max(3, min(args.steps, 20))         # as many steps as the headline by default: the pipeline's fill and drain are inside the timed region
            for name in ("cfg2", "cfg4", "zigbee1"):
                nn = int(WORKLOADS[name][3])
                r, _ = run_workload(name, nn, k, 1, device, 0, 1, checks=not args.no_cpu,
                                    parity_samples=0 if args.no_cpu else (nn if (name in PARITY_FULL and args.parity != "prefix")
                                                                          else int(CPU_SAMPLES[name]) // 4))
                others[name] = {f: r[f] for f in r if f in ("workload", "value", "unit", "ms_per_step", "steps", "kernel",
                                                  "kernel_ms", "frac", "step_frac", "achieved_GBps", "packets_per_gpu",
                                                  "decoded_crc_ok_per_gpu", "min_expected_crc_ok_per_gpu", "parity_in_run",
                                                  "frames_lost_vs_sequential")}
                if "fp32" in r:
                    others[name]["fp32_frac"] = r["fp32"]["frac"]
            r5 = cfg5_run(k, 3, not args.no_cpu)
            others["cfg5"] = {f: r5[f] for f in CFG5_FIELDS if f in r5}
            others["cfg5"]["note"] = "BASELINE.json configs[4] on one GPU; `--gpus N` carries its N-rank point the same way"
            out["other_workloads"] = others
        elif world > 1 and args.workload is None and not args.no_others:
            # configs[4] on the N ranks: segments round-robin, per-step RCCL all_gather of the records, dedup on rank 0
            r5 = cfg5_run(max(3, min(args.steps, 20)), 3, not args.no_cpu)
            if rank == 0:
                out["other_workloads"] = {"cfg5": {f: r5[f] for f in CFG5_FIELDS if f in r5}}
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0 and args.dump_outputs is not None:
        out["dumped_outputs"] = dump_outputs(args.dump_outputs, dump)
    if rank == 0:
        # RCCL prints its version banner through C stdio, which would otherwise be flushed at exit, after the JSON:
        # the JSON is the last line on stdout
        sys.stdout.flush()
        C.CDLL(None).fflush(None)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
