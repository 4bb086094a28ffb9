"""Z-Wave R2 on the MI355X (-m gpu): libsnout_rx.so's SNOUT_PROTO_ZWAVE path against tests/zwave_ref.py, the independent
numpy statement of z1-z7, bit for bit -- the soft taps, and every field of every record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from snout_amd import _ffi, zwave
import zwave_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIELDS = ("sample_index", "proto", "channel", "len", "crc_ok", "lqi", "pdu_type", "flags", "aux")


def _rx(**kw):
    from snout_amd.rx import SnoutRx
    return SnoutRx(proto=_ffi.PROTO_ZWAVE, device=0, **kw)


def _golden():
    x = np.fromfile(os.path.join(GOLD, "zwave_r2_800k.cf32"), dtype=np.complex64)
    doc = json.load(open(os.path.join(GOLD, "zwave_r2_expected.json")))
    return x, doc


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for k in FIELDS:
            assert int(g[k]) == int(w[k]), (k, int(g[k]), int(w[k]))
        b = bytes(g["bytes"])
        assert b[:w["len"]] == w["bytes"] and b[w["len"]:] == bytes(136 - w["len"])


def _quantize(x, fmt):
    """cf32 -> interleaved int8 / int16 and the cf32 capture it stands for (v 2^-7 / v 2^-15, exact)."""
    scale = 128.0 if fmt == 1 else 32768.0
    dt = np.int8 if fmt == 1 else np.int16
    lim = 127 if fmt == 1 else 32767
    iv = np.clip(np.rint(x.view(np.float32) * (scale / 2)), -lim, lim).astype(dt)
    back = (iv.astype(np.float32) / np.float32(scale)).view(np.complex64)
    return iv, back


def test_golden_file_gives_the_expected_frames(oracle):
    x, doc = _golden()
    with _rx() as rx:
        got = rx.process(x)
    sent = [bytes.fromhex(f["mpdu"]) for f in doc["frames"]]
    good = [bytes(p["bytes"][:p["len"]]) for p in got if p["crc_ok"]]
    assert good == sent
    want, _, _ = ref.receive(x, oracle.zb_mmse_taps())
    _same(got, want)


def test_soft_taps_are_bit_equal_to_the_checker(oracle):
    x, _ = zwave.capture(1 << 18, seed=5)
    with _rx() as rx:
        rx.process(x)
        f_gpu = rx.soft(_ffi.STAGE_ZW_FILTERED, 0, cap=1 << 20)
        syms = [rx.soft(_ffi.STAGE_ZW_SYMBOLS, lane, cap=1 << 20) for lane in range(3)]
    f, _, _ = ref.front(x)
    assert f_gpu.size == f.size and np.array_equal(f_gpu.view(np.uint32), f.view(np.uint32))
    core, warm = ref.lane_defaults()
    _, want = ref.lanes(f, oracle.zb_mmse_taps(), core, warm)
    for lane in range(3):
        assert syms[lane].size == want[lane].size > 1000
        assert np.array_equal(syms[lane].view(np.uint32), want[lane].view(np.uint32))


@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("log2n", [17, 20, 22])
def test_records_equal_the_checker_lane_mode(oracle, fmt, log2n):
    if fmt and log2n == 22:
        pytest.skip("integer formats: the 2^17 and 2^20 captures")
    x, truth = zwave.capture(1 << log2n, seed=log2n + 10 * fmt, sigma=0.08)
    if fmt:
        iv, x = _quantize(x, fmt)
    with _rx(channel=3, sample_format=fmt) as rx:
        got = rx.process(iv if fmt else x, first_sample_index=777)
    want, _, _ = ref.receive(x, oracle.zb_mmse_taps(), first=777, channel=3)
    _same(got, want)
    assert sum(1 for p in got if p["crc_ok"]) >= 0.8 * len(truth) > 0


def test_non_default_lane_shape_and_a_capture_shorter_than_a_core(oracle):
    x, _ = zwave.capture(1 << 19, seed=44)
    with _rx(zb_core=20000, zb_warmup=12000) as rx:
        got = rx.process(x)
    want, _, _ = ref.receive(x, oracle.zb_mmse_taps(), core=20000, warmup=12000)
    _same(got, want)
    assert len(set(int(p["aux"]) for p in got)) > 5
    short = x[:20000]
    with _rx() as rx:
        got = rx.process(short)
    want, _, _ = ref.receive(short, oracle.zb_mmse_taps())
    _same(got, want)
    assert len(got) >= 1


def test_submit_collect_gives_the_records_of_process():
    import torch
    xs = [zwave.capture(1 << 20, seed=60 + k)[0] for k in range(4)]
    with _rx() as rx:
        want = [rx.process(x, first_sample_index=k << 20) for k, x in enumerate(xs)]
        ts = [torch.from_numpy(x.view(np.float32)).cuda() for x in xs]
        got = []
        for k, t in enumerate(ts):
            rx.submit(t, first_sample_index=k << 20)
            if k >= 2:
                got.append(rx.collect())
        while len(got) < len(ts):
            got.append(rx.collect())
        prof = rx.profile()
        hist = rx.profile_history()
    for g, w in zip(got, want):
        assert g.tobytes() == w.tobytes() and len(w) > 0
    assert prof.dominant_name == "zw_front" and prof.ms_dominant > 0 and hist.size >= 8


def test_capacity_grows_when_a_lane_holds_more_frames_than_provisioned(oracle):
    x, _ = zwave.capture(1 << 20, seed=71, mean_gap=300.0, max_frames=None)
    with _rx(zb_core=200000, zb_warmup=16384) as rx:
        got = rx.process(x)
    want, _, _ = ref.receive(x, oracle.zb_mmse_taps(), core=200000, warmup=16384)
    _same(got, want)
    assert max(np.bincount(got["aux"].astype(np.int64))) > 16


def test_sixteen_channels_is_an_invalid_configuration():
    from snout_amd.rx import SnoutRx
    with pytest.raises(_ffi.SnoutError) as e:
        SnoutRx(proto=_ffi.PROTO_ZWAVE, n_channels=16, device=0)
    assert e.value.code == -1


def _cli(args, stdin=None):
    return subprocess.run([sys.executable, "-m", "snout_amd", "zwave", "scan"] + args, cwd=ROOT, input=stdin,
                          capture_output=True, timeout=300)


def test_cli_scan_of_the_golden_file_from_a_file_and_from_stdin():
    path = os.path.join(GOLD, "zwave_r2_800k.cf32")
    _, doc = _golden()
    sent = [f["mpdu"] for f in doc["frames"]]
    r = _cli(["--iq", path, "-t", "100"])
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().splitlines()
    assert [ln.split()[-1] for ln in lines] == sent
    assert all("908.40MHz" in ln for ln in lines)
    r2 = _cli(["--iq", "-", "-t", "100"], stdin=open(path, "rb").read())
    assert r2.returncode == 0, r2.stderr.decode()
    assert [ln.split()[-1] for ln in r2.stdout.decode().splitlines()] == sent
