"""GPU: bench.py's contract — one JSON line with the required keys at N = 1 (headline cfg #3 with
`roofline`, `cpu_baseline` and `other_workloads`), and the multi-rank orchestration of cfg #5 (rank
env, segments dealt round-robin, per-step record gather + de-duplication on rank 0, barrier, max over
ranks) with two ranks.  The box has one GPU, so the two ranks share it and talk over gloo
(SNOUT_BENCH_BACKEND): a check of the code path, not a measurement."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}
METRIC = json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]


def _last_json(out: bytes) -> dict:
    lines = [ln for ln in out.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.decode()[-2000:]
    return json.loads(lines[0])


def _bench(*args, env=None, timeout=900):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True,
                       timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return _last_json(r.stdout)


def test_headline_is_the_wideband_metric():
    d = _bench("--steps", "3", "--warmup", "1", "--samples", "4e7", "--cpu-samples", "4e6", "--no-others")
    assert KEYS <= set(d) and d["metric"] == METRIC                       # BASELINE.json's string, unchanged
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["config"]["workload"].startswith("cfg3")
    c = d["config"]
    assert c["decoded_crc_ok_per_gpu"] >= c["min_expected_crc_ok_per_gpu"] > 0
    rf = d["roofline"]
    assert rf["kernel"] == "pfb_spec40" and rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0 < rf["frac"] < 1
    assert abs(rf["algorithmic_bytes"] - (8 * 4e7 + 160 * c["packets_per_gpu"])) < 1
    assert 2000 < rf["measured_read_GBps"] < 8000 and rf["frac_of_measured_read"] > rf["frac"]
    assert 0 < rf["fp32"]["frac"] < 1 and rf["fp32"]["peak_TFLOPs"] == 157.3 and 181 < rf["fp32"]["flop_per_sample"] < 182
    assert rf["fp32_frac"] == rf["fp32"]["frac"]                          # flat copy for the driver's parser
    # parity in the same run: the records of the CPU leg's samples against the HIP path's, set equality
    pr = d["parity_in_run"]
    assert pr["equal"] is True and pr["workload"] == "cfg3" and pr["samples"] == 40000000 and pr["whole_capture"] is True
    assert pr["records"] > 1000 and pr["cpu_leg_prefix"]["equal"] is True and pr["cpu_leg_prefix"]["samples"] == 4000000
    assert rf["traffic"] is None                                           # the PMC figure is for the full-size workload
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and d["value"] > 20 * cb["value"]
    assert cb["all_cores"]["cores"] == cb["nproc"] >= 1 and cb["all_cores"]["value"] > 0 and cb["cpu_model"]


def test_default_run_carries_every_workload():
    d = _bench("--steps", "3", "--warmup", "1", timeout=1500)
    assert d["config"]["samples_per_gpu"] == 800000000 and "cpu_baseline" in d
    ow = d["other_workloads"]
    assert set(ow) == {"cfg2", "cfg4", "zigbee1", "cfg5"}
    for name, kern in (("cfg2", "btle_demod_corr"), ("cfg4", "pfb_spec16"), ("zigbee1", "zb_discrim..zb_walk")):
        w = ow[name]
        assert w["kernel"] == kern and w["value"] > 0 and w["kernel_ms"] > 0 and 0 < w["frac"] < 1
        assert w["decoded_crc_ok_per_gpu"] >= w["min_expected_crc_ok_per_gpu"] > 0
        assert w["parity_in_run"]["equal"] is True and w["parity_in_run"]["records"] > 100
    # the 802.15.4 steps are timed on the faithful default: what it loses against one sequential lane per channel, in-run
    for name, prefix, distinct in (("cfg4", 1 << 26, 3000), ("zigbee1", 1 << 24, 400)):
        fl = ow[name]["frames_lost_vs_sequential"]
        # (lost: frames of the sequential loop that the default decode misses; extra: FCS-ok frames, all of them transmitted,
        #  that the sequential loop itself misses -- its lock point at a preamble depends on thousands of samples of history.
        #  The prefix spans the capture's 32 distinct tiles: every frame counted is a different frame.  Measured on cfg #4:
        #  0.3 % lost + 0.7 % extra of 3 497)
        assert fl["samples"] == prefix and fl["distinct_sequential_frames"] > distinct
        assert fl["frac_lost"] <= 0.008 and fl["frac_lost_plus_extra"] <= 0.02
        fm = fl["fidelity_modes"]
        assert set(fm) == {"6144 / 3072 (default)" if name == "cfg4" else "6144 / 1024 (default)", "16384 / 8192", "one lane per channel"}
        # what exactness costs: the long lanes differ by less and take longer; one lane per channel IS the reference's loop
        assert fm["16384 / 8192"]["frac_lost_plus_extra"] <= max(0.006, fl["frac_lost_plus_extra"])
        assert fm["16384 / 8192"]["ms_per_step"] > 0 and fm["one lane per channel"]["Msamples_per_s"] > 0
        assert 0 < ow[name]["step_frac"] <= ow[name]["frac"] * 1.5
    assert ow["zigbee1"]["parity_in_run"]["samples"] == 1000000000 and ow["zigbee1"]["parity_in_run"]["whole_capture"] is True
    # the WHOLE 8e8-sample capture against the oracle (one segment, every host thread), and the timed CPU leg's prefix
    pr = d["parity_in_run"]
    assert pr["equal"] is True and pr["samples"] == 800000000 and pr["whole_capture"] is True and pr["records"] == d["config"]["packets_per_gpu"]
    assert pr["cpu_leg_prefix"]["equal"] is True and pr["cpu_leg_prefix"]["samples"] == 40 * (1 << 21)
    assert ow["cfg2"]["parity_in_run"]["samples"] == 1000000000 and ow["cfg4"]["parity_in_run"]["samples"] == 320000000
    assert ow["cfg2"]["parity_in_run"]["records"] == ow["cfg2"]["packets_per_gpu"]
    assert ow["cfg5"]["segments_per_gpu"] == 48 + 20 and ow["cfg5"]["decoded_crc_ok"] >= ow["cfg5"]["min_expected_crc_ok"] > 0
    assert ow["cfg5"]["segments_per_submission"] == {"btle": 48, "zigbee": 20}


def test_two_ranks_run_cfg5_over_gloo():
    """`--gpus N --workload cfg5` = BASELINE.json configs[4]: both wideband scans, segments round-robin over the ranks,
    records gathered and de-duplicated on rank 0 inside the timed region."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SNOUT_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg5", "--steps", "2", "--warmup", "1",
                        "--seconds", "1"], capture_output=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and "cpu_baseline" not in d      # the CPU baseline is timed at N = 1 only
    assert d["metric"] == METRIC and d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    c = d["config"]
    assert c["workload"].startswith("cfg5") and c["samples_per_gpu"] == 80000000 + 32000000
    assert c["decoded_crc_ok"] >= c["min_expected_crc_ok"] > 0 and "gloo" in c["sharding"]
    # record-exact at world 2: every rank's oracle records, gathered, de-duplicated == rank 0's GPU records
    pr = c["parity_in_run"]
    assert pr["ranks"] == 2 and pr["btle"]["equal"] is True and pr["zigbee"]["equal"] is True
    assert pr["btle"]["records"] + pr["zigbee"]["records"] == c["records_on_rank0"] > 2000


def test_two_ranks_default_line_is_the_headline_workload_on_every_rank():
    """`--gpus N` without a workload: cfg #3 on every rank (the N = 1 workload, so the driver's value(N) / (N value(1))
    is a scaling efficiency), per-step record gather to rank 0, and configs[4] on the same ranks in other_workloads."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SNOUT_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--samples", "4e7", "--seconds", "1"], capture_output=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and d["metric"] == METRIC and d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d
    c = d["config"]
    assert c["workload"].startswith("cfg3") and c["samples_per_gpu"] == 40000000 and "gather" in c["sharding"]
    assert c["ranks_in_collective"] == 2 and c["records_on_rank0_last_step"] >= 1.8 * c["decoded_crc_ok_per_gpu"]
    assert c["decoded_crc_ok_per_gpu"] >= c["min_expected_crc_ok_per_gpu"] > 0
    assert d["roofline"]["kernel"] == "pfb_spec40" and 0 < d["roofline"]["frac"] < 1
    o5 = d["other_workloads"]["cfg5"]
    assert o5["workload"].startswith("cfg5") and o5["decoded_crc_ok"] >= o5["min_expected_crc_ok"] > 0 and o5["value"] > 0


def test_cfg5_is_checked_against_the_oracle_as_cfg5():
    """`--workload cfg5` at reduced size (1 s of each band: 5 + 2 segments of 2^24 samples) -- rank 0's sorted,
    de-duplicated records of one step equal what the CPU oracle decodes from the same overlapping segments (+ the host statement
    of the de-duplication rule), every field and byte; the bench asserts it in-run and reports it."""
    d = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1")
    pr = d["config"]["parity_in_run"]
    assert pr["btle"]["equal"] is True and pr["zigbee"]["equal"] is True
    assert pr["btle"]["segments_per_rank"] == 5 and pr["zigbee"]["segments_per_rank"] == 2 and pr["ranks"] == 1
    assert pr["btle"]["records"] + pr["zigbee"]["records"] == d["config"]["records_on_rank0"] > 1000
    fl = d["config"]["frames_lost_vs_sequential"]
    assert fl["sequential_frames"] > 300 and fl["frac_lost"] <= 0.01


def test_four_ranks_decode_what_the_oracle_decodes():
    """`python3 bench.py --gpus 4 --workload cfg5 --seconds 0.9` -- the self-launched ranks, four of
    them (sharing the box's one GPU over gloo: a check of the code path, not a measurement; every rank and this test's own
    process hold the GPU, and four ranks keep that count at five), 0.9 s of each band per rank: the segments of 2^24 samples
    dealt round-robin and unevenly in both bands (BTLE 5 / 5 / 4 / 4, 802.15.4 2 / 2 / 2 / 1), so that ranks with fewer
    segments than rank 0 take part.  Rank 0's sorted, de-duplicated records of the last step == the CPU oracle run by every
    rank on ITS segments, gathered and de-duplicated by the host rule: every field and byte (asserted in-run)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SNOUT_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--workload", "cfg5", "--seconds", "0.9",
                        "--steps", "2", "--warmup", "1"], capture_output=True, timeout=1800, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = _last_json(r.stdout)
    c = d["config"]
    assert d["n_gpus"] == 4 and c["ranks_in_collective"] == 4 and c["workload"].startswith("cfg5")
    pr = c["parity_in_run"]
    assert pr["ranks"] == 4 and pr["btle"]["equal"] is True and pr["zigbee"]["equal"] is True
    assert pr["btle"]["segments_per_rank"] == 5 and pr["zigbee"]["segments_per_rank"] == 2      # rank 0's: the others hold fewer
    assert pr["btle"]["records"] + pr["zigbee"]["records"] == c["records_on_rank0"] > 3600
    assert c["decoded_crc_ok"] >= c["min_expected_crc_ok"] > 0


def test_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2 ...` as a plain command (no torchrun around it, WORLD_SIZE unset) starts
    its ranks as a child process and prints rank 0's JSON as the one JSON line, last on stdout.  Two ranks over gloo on the
    box's one GPU; the exchange is the real one (32-byte headers all_gather + records to rank 0)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SNOUT_BENCH_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--samples", "4e7", "--no-others"], capture_output=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = _last_json(r.stdout)
    assert r.stdout.decode().rstrip().splitlines()[-1].startswith("{")         # the JSON is the last line
    c = d["config"]
    assert KEYS <= set(d) and d["metric"] == METRIC and d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert c["ranks_in_collective"] == 2 and c["workload"].startswith("cfg3")
    # rank 0 holds every rank's records of the last step: the sum of what the two ranks decode (bench.py asserts equality
    # with the all-reduced count inside the run; both ranks decode >= the expected minimum)
    assert c["records_on_rank0_last_step"] >= 2 * c["min_expected_crc_ok_per_gpu"] > 0
    # on the RCCL backend one rank per GPU is required: asking for more GPUs than the box has fails fast, before any rank starts
    env.pop("SNOUT_BENCH_BACKEND")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1"], capture_output=True,
                       timeout=300, env=env)
    assert r.returncode == 2 and b"GPU(s) visible" in r.stderr and not r.stdout.strip()


def test_two_ranks_single_workload_over_gloo():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, SNOUT_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                        "--workload", "cfg2", "--samples", "6e7"], capture_output=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["samples_per_gpu"] == 60000000 and d["value"] > 0


@pytest.mark.parametrize("workload,samples,cpu,name", [
    ("cfg2", 6e7, 2e7, "btle_demod_corr"),
    ("cfg4", 16 * (1 << 19), 16 * (1 << 17), "pfb_spec16"),
    ("zigbee1", 1 << 23, 1 << 21, "zb_discrim..zb_walk"),
])
def test_other_workloads_keep_the_contract(workload, samples, cpu, name):
    d = _bench("--workload", workload, "--steps", "3", "--warmup", "1", "--samples", str(samples),
               "--cpu-samples", str(cpu))
    assert KEYS <= set(d) and d["config"]["workload"].startswith(workload.replace("zigbee1", "single-channel 802"))
    assert d["roofline"]["kernel"] == name and 0 < d["roofline"]["frac"] < 1 and d["roofline"]["traffic"] is None
    c = d["config"]
    assert c["decoded_crc_ok_per_gpu"] >= c["min_expected_crc_ok_per_gpu"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["value"] > d["cpu_baseline"]["value"]
    assert d["parity_in_run"]["equal"] is True and d["parity_in_run"]["workload"] == workload


def test_integer_input_format_line():
    d = _bench("--workload", "cfg2", "--format", "sc8", "--steps", "3", "--warmup", "1", "--samples", "6e7",
               "--cpu-samples", "2e7")
    assert KEYS <= set(d) and d["dtype"] == "i8->i32" and "sc8" in d["config"]["workload"]
    # 2 B per sample: the algorithmic bytes of the roofline follow the format
    assert abs(d["roofline"]["algorithmic_bytes"] - (2 * 6e7 + 160 * d["config"]["packets_per_gpu"])) < 1
    assert d["config"]["decoded_crc_ok_per_gpu"] >= d["config"]["min_expected_crc_ok_per_gpu"] > 0


def test_cfg5_exchange_runs_on_rccl_at_world_one():
    """with SNOUT_BENCH_NCCL1=1 a one-GPU box initialises the nccl (= RCCL) backend at world size
    1, so cfg #5's per-step all_gather_into_tensor on device buffers, the device-side dedup behind it and the
    device-side packing of the records execute exactly as they will on 8 GPUs."""
    env = dict(os.environ, SNOUT_BENCH_NCCL1="1")
    d = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1", env=env)
    c = d["config"]
    assert c["collective"].startswith("RCCL all_gather (32-B headers) + gather to rank 0") and c["ranks_in_collective"] == 1 and c["device_of_rank0"] == 0
    assert "RCCL" in c["sharding"] and c["decoded_crc_ok"] >= c["min_expected_crc_ok"] > 0
    plain = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1")
    assert plain["config"]["collective"].startswith("none") and plain["config"]["decoded_crc_ok"] == c["decoded_crc_ok"]
    assert plain["config"]["records_on_rank0"] == c["records_on_rank0"]


def test_headline_exchange_runs_on_rccl_at_world_one():
    """What `--gpus N` times at N > 1 — cfg #3 with the per-step gather of the records — on a real RCCL collective at
    world size 1 (SNOUT_BENCH_NCCL1=1): rank 0 receives exactly the records it decoded."""
    env = dict(os.environ, SNOUT_BENCH_NCCL1="1")
    d = _bench("--workload", "cfg3", "--steps", "3", "--warmup", "1", "--samples", "4e7", "--no-cpu", env=env)
    c = d["config"]
    assert c["collective"].startswith("RCCL all_gather (32-B headers) + gather to rank 0") and c["ranks_in_collective"] == 1 and "nccl" in c["sharding"]
    assert c["records_on_rank0_last_step"] == c["packets_per_gpu"] > 0
    assert c["decoded_crc_ok_per_gpu"] >= c["min_expected_crc_ok_per_gpu"] > 0


def test_rank0_load_of_eight_ranks_is_rehearsed_at_world_one():
    """`SNOUT_BENCH_FAKE_WORLD=8` on the RCCL backend at world size 1 -- after the real exchange rank 0
    holds EIGHT blocks of records (its own, sample_index shifted per block), sorts / de-duplicates them on the GPU and
    downloads them inside the timed region, as rank 0 of an 8-GPU run will.  Both bench paths: cfg #5 (device dedup) and
    the headline workload with its per-step gather."""
    env = dict(os.environ, SNOUT_BENCH_NCCL1="1", SNOUT_BENCH_FAKE_WORLD="8")
    plain = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1", env=dict(os.environ, SNOUT_BENCH_NCCL1="1"))
    d = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1", env=env)
    c, p = d["config"], plain["config"]
    assert c["fake_world"]["blocks_on_rank0"] == 8 and c["records_on_rank0"] == 8 * p["records_on_rank0"]
    assert c["decoded_crc_ok"] == 8 * p["decoded_crc_ok"] and c["collective"].startswith("RCCL")
    h = _bench("--workload", "cfg3", "--steps", "3", "--warmup", "1", "--samples", "4e7", "--no-cpu", env=env)
    assert h["config"]["fake_world"] == 8 and h["config"]["records_on_rank0_last_step"] == 8 * h["config"]["packets_per_gpu"] > 0


def test_dump_outputs_are_the_last_steps_records_and_repeat(tmp_path):
    """`--dump-outputs DIR`: the records of the last timed step, every field as a float array in DIR; the same arguments
    give the same capture, so a second run writes the same arrays (two builds can be compared output for output)."""
    import numpy as np
    args = ("--steps", "2", "--warmup", "1", "--samples", "4e7", "--no-cpu", "--no-others")
    runs = []
    for k in range(2):
        d = _bench(*args, "--dump-outputs", str(tmp_path / str(k)))
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        n = d["config"]["packets_per_gpu"]
        assert d["dumped_outputs"]["records"] == {"records": n} and d["dumped_outputs"]["rows_written"] == {"records": n}
        runs.append({p.name: np.load(p) for p in (tmp_path / str(k)).iterdir()})
    a, b = runs
    assert set(a) == set(b) and "records_sample_index.npy" in a and a["records_bytes.npy"].shape == (n, 136)
    assert sum(v.nbytes for v in a.values()) < 64e6 and all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert int(a["records_crc_ok.npy"].sum()) >= d["config"]["min_expected_crc_ok_per_gpu"] > 0
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    # cfg #5: both scans' records of the last step, as rank 0 holds them
    d = _bench("--workload", "cfg5", "--steps", "2", "--warmup", "1", "--seconds", "1", "--no-cpu",
               "--dump-outputs", str(tmp_path / "cfg5"))
    recs = d["dumped_outputs"]["records"]
    assert set(recs) == {"btle_records", "zigbee_records"} and sum(recs.values()) == d["config"]["records_on_rank0"]
    for name, n in recs.items():
        assert np.load(tmp_path / "cfg5" / f"{name}_channel.npy").shape == (n,)
