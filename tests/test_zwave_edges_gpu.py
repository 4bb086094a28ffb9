"""Z-Wave R2 on the MI355X (-m gpu), at the edges: lengths that are not multiples of the kernels' vector width or tiles,
lane shapes with more lanes than zw_scan has threads, non-finite and extreme samples, the squelch at its threshold, the
integer formats' extremes, record fields at their limits, the pipelined calls, and scans longer than one segment.
Everything is compared with tests/zwave_ref.py bit for bit: the FILTERED tap as uint32, every record field and byte."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from snout_amd import _ffi, zwave
import zwave_cuts as cuts
import zwave_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIELDS = ("sample_index", "proto", "channel", "len", "crc_ok", "lqi", "pdu_type", "flags", "aux")
CORE, WARM = ref.lane_defaults()


def _rx(**kw):
    from snout_amd.rx import SnoutRx
    return SnoutRx(proto=_ffi.PROTO_ZWAVE, device=0, **kw)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in FIELDS:
            assert int(g[k]) == int(w[k]), (k, int(g[k]), int(w[k]))
        b = bytes(g["bytes"])
        assert b[:w["len"]] == w["bytes"] and b[w["len"]:] == bytes(136 - w["len"])


def _bits_equal(a, b):
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _run(x, mmse, core=0, warmup=0, first=0, channel=0, fmt=0, xin=None, sequential=False):
    """The GPU's records and FILTERED tap against the checker's (bit-exact); returns the checker's records."""
    kw = dict(zb_core=core, zb_warmup=warmup) if core or warmup else {}
    with _rx(channel=channel, sample_format=fmt, **kw) as rx:
        got = rx.process(x if xin is None else xin, first_sample_index=first)
        f_gpu = rx.soft(_ffi.STAGE_ZW_FILTERED, 0, cap=max(len(x), 1) + 64)
    with np.errstate(all="ignore"):
        want, f, _ = ref.receive(x, mmse, core=core, warmup=warmup, first=first, channel=channel,
                                 sequential=sequential)
    assert _bits_equal(f_gpu, f)
    assert np.all(np.isfinite(f_gpu))
    _same(got, want)
    return want


# --- lengths -----------------------------------------------------------------------------------------------------------

LENGTHS = [0, 1, 8, 9, 38, 39, 40, 192, 193, 231, 232, 1000, 2047, 2048, 2049, 2048 + 231, 4097, 32767, 32768, 32769,
           32768 + 7, 32768 + 8, (1 << 20) + 5]


def test_lengths_reach_the_tail_store_and_short_last_lanes():
    assert any(n >= 9 and n % 8 for n in LENGTHS)                            # zw_front's scalar tail store
    last = [n - (n - 1) // CORE * CORE for n in LENGTHS if n > CORE]         # samples in the last lane
    assert any(1 <= m <= 7 for m in last) and 8 in last


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths(oracle, n):
    x, _ = zwave.capture(max(n, 1), seed=300 + n % 97, mean_gap=2000.0)
    x = x[:n]
    if n < 9:
        with _rx() as rx:
            assert len(rx.process(x)) == 0
            with pytest.raises(_ffi.SnoutError):
                rx.soft(_ffi.STAGE_ZW_FILTERED, 0, cap=64)
        return
    want = _run(x, oracle.zb_mmse_taps(), first=n)
    if n >= 1 << 20:
        assert len(want) > 50


# --- non-finite, overflowing and tiny samples ----------------------------------------------------------------------------

def test_non_finite_and_extreme_cf32(oracle):
    x, truth = zwave.capture(1 << 18, seed=8, sigma=0.02, mean_gap=3000.0)
    v = x.view(np.float32).reshape(-1, 2)
    k = 3000
    for comp in ([0], [1], [0, 1]):                                      # isolated NaN, +Inf, -Inf in either and both
        for val in (np.nan, np.inf, -np.inf):
            v[k, comp] = val
            k += 7001
    v[k:k + 100, :] = 3e38                                               # z1 overflows to Inf, |y|^2 too
    v[k + 9000:k + 9040, 0] = -3e38
    v[k + 20000:k + 20300, :] = 1e-40                                    # denormals
    v[k + 30000:k + 30200, :] = -0.0
    v[k + 40000:k + 41000, :] = 0.0
    assert k + 41000 < x.size and not np.all(np.isfinite(v))
    want = _run(x, oracle.zb_mmse_taps())
    assert sum(r["crc_ok"] for r in want) >= len(truth) // 2


# --- the squelch at its threshold ----------------------------------------------------------------------------------------

def test_squelch_decisions_at_the_threshold(oracle):
    """A tone at -195 kHz whose amplitude ramps 0.009 -> 0.011 -> 0.009: the filtered power crosses 1e-4 twice."""
    n = 1 << 18
    i = np.arange(n)
    amp = np.interp(i, [0, n // 2, n], [0.009, 0.011, 0.009])
    x = (amp * np.exp(1j * (0.3 + 2 * np.pi * (-195e3) / 800e3 * i))).astype(np.complex64)
    # the checker's z1 output before the squelch (the same mixing and FIR as ref.front)
    h1, _ = ref.taps()
    F = np.float32
    r = i & 3
    re_, im_ = x.real.astype(F), x.imag.astype(F)
    ur = np.select([r == 0, r == 1, r == 2, r == 3], [re_, -im_, -re_, im_]).astype(F)
    ui = np.select([r == 0, r == 1, r == 2, r == 3], [im_, re_, -im_, -re_]).astype(F)
    yr, yi = ref._fir(ur, h1), ref._fir(ui, h1)
    p = ((yr * yr).astype(F) + (yi * yi).astype(F)).astype(F).astype(np.float64)[39:]
    near = np.abs(p / 1e-4 - 1) <= 1e-3
    assert near.sum() >= 300 and (p[near] >= 1e-4).sum() >= 100 and (p[near] < 1e-4).sum() >= 100
    _, y, _ = ref.front(x)
    assert np.array_equal(y[39:] != 0, p >= 1e-4)
    _run(x, oracle.zb_mmse_taps())


@pytest.mark.parametrize("khz, amp, want", [(-20, 1.0, -16.0), (5, 1.0, 4.0), (30, 1.0, 24.0), (-250, 5.0, 0.0),
                                             (300, 1.0, 0.0), (5, 0.005, 0.0), (-20, 0.02, -16.0)])
def test_tones_give_the_known_answers(oracle, khz, amp, want):
    """tests/test_zwave_float64.py's known answers on the GPU: a tone at -200 kHz + d gives f = d / 1250 after the
    232-sample transient when the squelch is open; out of the channel or too weak, exactly 0."""
    n = 8192
    x = (amp * np.exp(1j * (0.3 + 2 * np.pi * (-200e3 + khz * 1e3) / 800e3 * np.arange(n)))).astype(np.complex64)
    _run(x, oracle.zb_mmse_taps())
    with _rx() as rx:
        rx.process(x)
        f = rx.soft(_ffi.STAGE_ZW_FILTERED, 0, cap=n)
    if want == 0.0:
        assert np.all(f[232:] == 0.0)
    else:
        assert np.max(np.abs(f[232:].astype(np.float64) - want)) <= 2e-3


# --- integer formats at their extremes -----------------------------------------------------------------------------------

def _quantize_full(x, fmt):
    """cf32 -> interleaved int8 / int16 reaching -128 / -32768 (round, then clip to the type's own range), and the cf32
    capture it stands for (v 2^-7 / v 2^-15, exact)."""
    scale = 128.0 if fmt == 1 else 32768.0
    dt = np.int8 if fmt == 1 else np.int16
    info = np.iinfo(dt)
    iv = np.clip(np.rint(x.view(np.float32) * scale), info.min, info.max).astype(dt)
    return iv, (iv.astype(np.float32) / np.float32(scale)).view(np.complex64)


@pytest.mark.parametrize("fmt", [1, 2])
def test_integer_extremes(oracle, fmt):
    n = 1 << 17
    rng = np.random.default_rng(40 + fmt)
    x, truth = zwave.capture(n, seed=40 + fmt, sigma=0.0, mean_gap=2500.0)
    x = x * np.complex64(1.2)                                             # frames past full scale: saturated both ways
    x[:8000] = (rng.uniform(-1.1, 1.1, 8000) + 1j * rng.uniform(-1.1, 1.1, 8000)).astype(np.complex64)
    sq = np.where((np.arange(4000) // 10) % 2, 1.5, -1.5)                 # a saturated square wave
    x[-4000:] = (sq + 1j * sq[::-1]).astype(np.complex64)
    iv, back = _quantize_full(x, fmt)
    lo, hi = np.iinfo(iv.dtype).min, np.iinfo(iv.dtype).max
    assert (iv == lo).sum() > 1000 and (iv == hi).sum() > 1000
    want = _run(back, oracle.zb_mmse_taps(), fmt=fmt, xin=iv)
    assert sum(r["crc_ok"] for r in want) >= len(truth) // 2 > 0


# --- lane shapes ---------------------------------------------------------------------------------------------------------

# a warm-up of 0 in snout_rx_cfg selects the default (16384): 1 is the shortest warm-up the ABI can state
SHAPES = [(1024, 1, 1 << 18), (1024, 1024, 1 << 18), (1024, 5120, 1 << 18), (1500, 700, 1 << 22),
          (1024, 512, 1 << 22), (32768, 1, 1 << 19), (40000, 1 << 24, 1 << 19)]


@pytest.mark.parametrize("core, warmup, n", SHAPES)
def test_lane_shapes(oracle, core, warmup, n):
    x, _ = zwave.capture(n, seed=core % 251 + warmup % 7, mean_gap=400.0 if n >= 1 << 22 else 1500.0)
    lanes = -(-n // core)
    want = _run(x, oracle.zb_mmse_taps(), core=core, warmup=warmup, channel=5)
    if n == 1 << 22:
        assert lanes > 1024                                               # zw_scan: several lanes per thread
        if core == 1500:
            assert lanes == 2797 and lanes % 1024
    aux = np.bincount([r["aux"] for r in want], minlength=lanes)
    assert (aux > 0).sum() > 3
    if core >= 20000:
        assert aux.max() >= 2            # (a frame is 4960 samples or more: a 1024- or 1500-sample core owns one at most)


def test_one_lane_is_the_sequential_receiver(oracle):
    x, _ = zwave.capture(1 << 19, seed=77)
    mm = oracle.zb_mmse_taps()
    want = _run(x, mm, core=1 << 20, sequential=True)
    seq, _, _ = ref.receive(x, mm, sequential=True)
    assert [r["bytes"] for r in want] == [r["bytes"] for r in seq] and len(want) > 10
    assert all(r["aux"] == 0 for r in want)
    import json
    g = np.fromfile(os.path.join(GOLD, "zwave_r2_800k.cf32"), dtype=np.complex64)
    doc = json.load(open(os.path.join(GOLD, "zwave_r2_expected.json")))
    want = _run(g, mm, core=g.size, sequential=True)
    assert [r["bytes"].hex() for r in want] == [fr["mpdu"] for fr in doc["frames"]]


@pytest.mark.parametrize("core, warmup, n", [(0, 0, 1 << 18), (20000, 3000, 1 << 18), (1 << 20, 0, 1 << 17)])
def test_symbols_tap_of_first_middle_last_lane(oracle, core, warmup, n):
    x, _ = zwave.capture(n, seed=91)
    mm = oracle.zb_mmse_taps()
    kw = dict(zb_core=core, zb_warmup=warmup) if core else {}
    c, w = (core, warmup) if core else (CORE, WARM)
    lanes = -(-n // c)
    pick = sorted({0, lanes // 2, lanes - 1})
    with _rx(**kw) as rx:
        rx.process(x)
        got = {k: rx.soft(_ffi.STAGE_ZW_SYMBOLS, k, cap=1 << 20) for k in pick}
        with pytest.raises(_ffi.SnoutError):
            rx.soft(_ffi.STAGE_ZW_SYMBOLS, lanes, cap=64)
    f, _, _ = ref.front(x)
    _, want = ref.lanes(f, mm, c, w)
    for k in pick:
        assert got[k].size > 50 and _bits_equal(got[k], want[k]), k


# --- record fields at their limits ---------------------------------------------------------------------------------------

def test_record_fields_at_their_limits(oracle):
    x, _ = zwave.capture(1 << 18, seed=12)
    first = (1 << 40) + 12345
    want = _run(x, oracle.zb_mmse_taps(), first=first, channel=0xFFFF)
    assert len(want) > 5 and all(r["sample_index"] > 1 << 40 and r["channel"] == 0xFFFF for r in want)


@pytest.mark.parametrize("channel", [0x10000, 70000, 0xFFFFFFFF])
def test_channel_labels_above_16_bits_are_refused(channel):
    with pytest.raises(_ffi.SnoutError) as e:
        _rx(channel=channel)
    assert e.value.code == -1                                             # SNOUT_EINVAL


# --- pipelined calls ------------------------------------------------------------------------------------------------------

def test_pipelined_submit_collect_with_a_capacity_rerun():
    import torch
    dense, _ = zwave.capture(1 << 20, seed=71, mean_gap=300.0)            # > 16 frames in one 200000-sample lane
    xs = [zwave.capture(1 << 19, seed=120 + k)[0] for k in range(2)] + [dense] + \
         [zwave.capture((1 << 19) + 3, seed=130 + k)[0] for k in range(2)]
    kw = dict(zb_core=200000, zb_warmup=16384)
    with _rx(**kw) as rx:
        want = [rx.process(x, first_sample_index=k << 21) for k, x in enumerate(xs)]
    assert max(np.bincount(want[2]["aux"].astype(np.int64))) > 16
    ts = [torch.from_numpy(x.view(np.float32)).cuda() for x in xs]
    with _rx(**kw) as rx:                                                 # a fresh handle: K starts small again
        got = []
        for k, t in enumerate(ts):
            rx.submit(t, first_sample_index=k << 21)
            if k >= 2:
                got.append(rx.collect())
        while len(got) < len(ts):
            got.append(rx.collect())
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes() and len(w) > 0


def test_records_on_the_device_are_the_records_of_a_plain_handle():
    import torch
    from snout_amd.dist import _device_bytes
    xs = [zwave.capture(1 << 19, seed=140 + k)[0] for k in range(3)]
    with _rx() as rx:
        want = [rx.process(x, first_sample_index=k << 19) for k, x in enumerate(xs)]
    ts = [torch.from_numpy(x.view(np.float32)).cuda() for x in xs]
    with _rx(records_on_device=True) as rx:
        for k, t in enumerate(ts):
            rx.submit(t, first_sample_index=k << 19)
        for k in range(len(ts)):
            n = rx.collect()
            ptr, m = rx.last_records_device()
            assert n == m == len(want[k]) > 0
            raw = _device_bytes(torch, ptr, m * _ffi.PKT_DTYPE.itemsize, ts[k].device).cpu().numpy()
            assert raw.tobytes() == want[k].tobytes()


# --- scans longer than one segment ----------------------------------------------------------------------------------------

def _kept_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _same(g, w)


@pytest.mark.parametrize("edge", [False, True])
def test_segments_against_their_composition(oracle, monkeypatch, edge):
    seg = 1 << 18
    monkeypatch.setattr(zwave, "SEGMENT", seg)
    n = 5 * seg - 12345
    c = cuts.file_cuts(n, seg)
    x, placed = cuts.placed_capture(c, n, seed=30, edge=edge)
    mm = oracle.zb_mmse_taps()
    got = list(zwave.segments(x, device=0, channel=4))
    want = cuts.compose(x, c, lambda ch, first: ref.receive(ch, mm, first=first, channel=4)[0])
    _kept_equal(got, want)
    assert [bytes(p["bytes"][:p["len"]]) for rec in got for p in rec if p["crc_ok"]] == [m for _, _, m in placed]


def _long_capture(cut):
    """Frames at every cut of a capture of three segments and a bit (tests/zwave_cuts.py, the real SEGMENT)."""
    n = 3 * zwave.SEGMENT + 99999
    c = cut(n, zwave.SEGMENT)
    x, placed = cuts.placed_capture(c, n, seed=30)
    assert len(c) == 4 and all(any(s0 < b < e for s0, e, _ in placed) for _, b, _ in c[:-1])   # frames across the cuts
    return x, [m for _, _, m in placed]


@pytest.mark.parametrize("fmt", [0, 1])
def test_scan_of_a_file_of_three_segments(tmp_path, fmt):
    from snout_amd.scan import FileSource
    x, sent = _long_capture(cuts.file_cuts)
    path = str(tmp_path / "z.iq")
    (_quantize_full(x, 1)[0] if fmt else x).tofile(path)
    scan = zwave.ZWaveScan(source=FileSource(path, fmt), timeout=None, device=0)
    assert [m.mpdu for m in scan.run()] == sent                          # every frame once, in capture order


def test_stream_source_against_its_composition(oracle):
    from snout_amd.scan import StreamSource
    seg = 150000
    n = 5 * seg
    c = cuts.stream_cuts(n, seg)
    assert len(c) >= 4
    x, placed = cuts.placed_capture(c, n, seed=30)
    mm = oracle.zb_mmse_taps()
    src = StreamSource(io.BytesIO(x.tobytes()), 0, segment=seg)
    got = list(src.segments(_ffi.PROTO_ZWAVE, 0, 0))
    want = cuts.compose(x, c, lambda ch, first: ref.receive(ch, mm, first=first)[0])
    _kept_equal(got, want)


def test_cli_scan_of_a_multi_segment_capture_from_stdin():
    x, sent = _long_capture(cuts.stream_cuts)
    r = subprocess.run([sys.executable, "-m", "snout_amd", "zwave", "scan", "--iq", "-", "-t", "1000"], cwd=ROOT,
                       input=x.tobytes(), capture_output=True, timeout=400)
    assert r.returncode == 0, r.stderr.decode()
    assert [ln.split()[-1] for ln in r.stdout.decode().splitlines()] == [m.hex() for m in sent]
