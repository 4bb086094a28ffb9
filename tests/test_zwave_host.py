"""Z-Wave R2 without a GPU: the frozen tap tables, the checksum and MPDU parse, the checker (tests/zwave_ref.py) on the
golden fixture in both modes, the lanes against the one sequential loop, the C ABI constants, the CLI surface, pcap."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from snout_amd import _ffi, zwave
from snout_amd.formats import read_pcap, write_pcap
import zwave_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_regenerated_taps_equal_the_committed_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_zwave_taps
    assert gen_zwave_taps.render() == open(os.path.join(ROOT, "snout_amd", "csrc", "zwave_taps.inc")).read()
    h1, h2 = ref.taps()
    assert h1.size == 39 and h2.size == 193
    assert np.array_equal(h1, h1[::-1]) and np.array_equal(h2, h2[::-1])        # linear phase
    assert abs(float(h1.astype(np.float64).sum()) - 1) < 1e-6 and abs(float(h2.astype(np.float64).sum()) - 1) < 1e-6


def test_checksum_and_parse_known_answers():
    # a NOP frame: HomeID 0xC0FFEE01, src 1, singlecast, ack requested, seq 5, L 10, dst 2
    body = bytes.fromhex("c0ffee0101410a0a02")
    assert zwave.checksum(body) == 0xFF ^ 0xC0 ^ 0xFF ^ 0xEE ^ 0x01 ^ 0x01 ^ 0x41 ^ 0x0A ^ 0x0A ^ 0x02
    m = zwave.make_mpdu(0xC0FFEE01, 1, 2, b"", header_type=1, seq=10, ack=True)
    assert m[:9] == bytes.fromhex("c0ffee0101410a0a02") and m[9] == zwave.checksum(m[:9])
    h = zwave.parse_mpdu(m)
    assert (h["home_id"], h["src"], h["dst"], h["header_type"], h["seq"]) == (0xC0FFEE01, 1, 2, 1, 10)
    assert (h["routed"], h["ack"], h["low_power"], h["payload"], h["checksum_ok"]) == (False, True, False, b"", True)
    m2 = zwave.make_mpdu(0x01020304, 7, 255, b"\x20\x01\xff", header_type=2, seq=3, routed=True, low_power=True)
    h2 = zwave.parse_mpdu(m2)
    assert h2["payload"] == b"\x20\x01\xff" and h2["routed"] and h2["low_power"] and not h2["ack"]
    assert h2["length"] == 13 and h2["header_type"] == 2
    bad = m2[:-1] + bytes([m2[-1] ^ 1])
    assert not zwave.parse_mpdu(bad)["checksum_ok"]
    with pytest.raises(ValueError):
        zwave.parse_mpdu(m2[:-1])


@pytest.mark.parametrize("sequential", [True, False])
def test_checker_decodes_every_golden_frame(oracle, sequential):
    x = np.fromfile(os.path.join(GOLD, "zwave_r2_800k.cf32"), dtype=np.complex64)
    doc = json.load(open(os.path.join(GOLD, "zwave_r2_expected.json")))
    assert x.size == doc["n_samples"] and len(doc["frames"]) >= 6
    recs, f, _ = ref.receive(x, oracle.zb_mmse_taps(), sequential=sequential)
    assert [r["bytes"].hex() for r in recs] == [fr["mpdu"] for fr in doc["frames"]]
    assert all(r["crc_ok"] == 1 and r["proto"] == 2 for r in recs)
    # the record's position: the SOF's last bit, through the filters' group delay (19 + 96 samples) and the loop's phase
    for r, fr in zip(recs, doc["frames"]):
        assert 0 <= r["sample_index"] - fr["sof_end"] <= 20 + 115


def test_lanes_against_the_one_sequential_loop(oracle):
    """>= 500 frames of three seeds (noise sigma 0.08, carrier offsets up to 500 Hz): the default lane shape against the
    sequential receiver.  A lane's timing loop locks at its own phase inside the flat middle of a symbol (DESIGN.md
    section 8), so positions agree within a symbol and a few frames differ (measured: 17 lost, 14 extra of 506)."""
    mm = oracle.zb_mmse_taps()
    core, warm = ref.lane_defaults()
    total = lost = extra = 0
    for seed in (101, 102, 103):
        x, _ = zwave.capture(170 * 14500, seed=seed, sigma=0.08, cfo_hz=500.0)
        f, _, _ = ref.front(x)
        seq, _ = ref.lanes(f, mm, f.size, 0)
        ln, _ = ref.lanes(f, mm, core, warm)
        total += len(seq)

        def near(p, qs):
            return any(p["bytes"] == q["bytes"] and abs(p["sample_index"] - q["sample_index"]) <= zwave.SPS for q in qs)
        lost += sum(not near(q, ln) for q in seq)
        extra += sum(not near(p, seq) for p in ln)
    assert total >= 500
    assert lost <= 0.05 * total and extra <= 0.05 * total, (total, lost, extra)


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "snout_rx.h")).read()
    val = lambda name: int(re.search(rf"#define {name}\s+(\d+)u", text).group(1))
    assert val("SNOUT_PROTO_ZWAVE") == _ffi.PROTO_ZWAVE == 2
    assert val("SNOUT_STAGE_ZW_FILTERED") == _ffi.STAGE_ZW_FILTERED
    assert val("SNOUT_STAGE_ZW_SYMBOLS") == _ffi.STAGE_ZW_SYMBOLS
    assert val("SNOUT_ABI_VERSION") == _ffi.ABI_VERSION == 4
    assert ref.lane_defaults() == (val("SNOUT_ZWAVE_LANE_CORE"), val("SNOUT_ZWAVE_LANE_WARMUP"))


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "snout_amd", "zwave", "scan", *args], cwd=ROOT, capture_output=True,
                          timeout=120)


def test_cli_help_and_missing_iq():
    r = _cli("--help")
    assert r.returncode == 0 and b"--lane-core" in r.stdout and b"--iq" in r.stdout
    r = _cli("-t", "1")
    assert r.returncode == 2 and b"--iq" in r.stderr


def test_pcap_with_the_zwave_linktype_reads_back(tmp_path):
    m = [zwave.make_mpdu(0xDEADBEEF, 1, 2, bytes(range(k))) for k in (0, 5, 54)]
    p = str(tmp_path / "z.pcap")
    assert write_pcap(p, [(1.5 + i, b) for i, b in enumerate(m)], linktype=zwave.LINKTYPE_ZWAVE_R1_R2) == 3
    lt, frames = read_pcap(p)
    assert lt == 261 and [b for _, b in frames] == m
