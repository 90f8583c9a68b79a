"""GPU parity tests at the FULL sizes of BASELINE.json `configs` (1, 3, 4), the fresh-output
contract of PWCDCNet.__call__, per-stream plans, and bench.py's self-spawned launch.

Tolerance: BASELINE.json north_star -- max-abs 1e-3 per flow component on flows_final (px).
The oracle is run on single pairs (seconds of CPU each); batches are checked pair-wise.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pa():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    import pwcnet_amd
    return pwcnet_amd


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# Bounds of flows_final against the float64 restatement (util.check_float64; pyramid levels against bound / 20), beside the
# fp32 oracle's 1e-3 px: max(10 x the worst error measured on an MI355X, 1e-5 px), as tests/test_gpu_model.py.
# Measured (px): see the comment at each entry.
F64_BOUND_PX = {
    "config1": 1.9e-5,          # 1.9e-6 (pair 0, pyramid)
    "config3": 6.4e-5,          # 6.3e-6 (single pair 0, pyramid)
    "config4": 1.8e-5,          # 1.8e-6 (pair 1)
    "config4_b8": 2.2e-5,       # 2.1e-6 (pair 7)
}


def make_net(pa, use_dc=False, **kw):
    w = util.model_weights(use_dc)
    net = pa.PWCDCNet(use_dc=use_dc, **kw)
    net.load_weights(w)
    return net, w


# ------------------------------------------------------------------ BASELINE configs at size
def test_config1_batch8_448x1024_winograd_pairs_vs_oracle(pa):
    """configs[1]: batch 8 at 448x1024 on the default (Winograd) path -- the N = 8 tile plans, not
    the single-pair ones: pairs 0 and 7 of the batch against the oracle run on those pairs."""
    net, w = make_net(pa, False)
    im0, im1 = util.smooth_images(8, 448, 1024, seed=41, shift=(5, -3))
    final, pyr = net(gpu(im0), gpu(im1))
    got = final.cpu().numpy()
    assert got.shape == (8, 448, 1024, 2)
    onet = orc.OraclePWCDCNet(w)
    for i in (0, 7):
        e_final, e_pyr = onet(im0[i:i + 1], im1[i:i + 1])
        err = float(np.abs(got[i:i + 1] - e_final).max())
        assert err <= 1e-3, (i, err)
        for p, e in zip(pyr, e_pyr):
            assert float(np.abs(p[i:i + 1].cpu().numpy() - e).max()) <= 5e-5
        util.check_float64(f"config1 pair {i}", got[i:i + 1], [p[i:i + 1] for p in pyr],
                           util.float64_flows(w, False, im0[i:i + 1], im1[i:i + 1]), F64_BOUND_PX["config1"])


def test_config3_dc_448x1024_vs_oracle_and_batch8(pa):
    """configs[3]: PWCDCNet use_dc=True at 448x1024 -- the 2717-channel first conv of level 4 and
    the 3165-channel context input at size; one pair against the oracle, then a batch of 8 in
    which pairs 0 and 7 must reproduce the single-pair runs."""
    net, w = make_net(pa, True)
    im0, im1 = util.smooth_images(8, 448, 1024, seed=42, shift=(4, 2))
    one, pyr1 = net(gpu(im0[:1]), gpu(im1[:1]))
    e_final, _ = orc.OraclePWCDCNet(w, use_dc=True)(im0[:1], im1[:1])
    err = float(np.abs(one.cpu().numpy() - e_final).max())
    assert err <= 1e-3, err
    util.check_float64("config3 single pair 0", one, pyr1, util.float64_flows(w, True, im0[:1], im1[:1]), F64_BOUND_PX["config3"])
    f8, pyr8 = net(gpu(im0), gpu(im1))
    assert f8.shape == (8, 448, 1024, 2)
    # different batch sizes may pick different tile plans (same arithmetic, other summation order)
    assert float((f8[0:1] - one).abs().max()) <= 2e-4
    # pair 7 of the batch against the ORACLE run on that pair (not against another HIP run)
    e7, _ = orc.OraclePWCDCNet(w, use_dc=True)(im0[7:8], im1[7:8])
    err7 = float(np.abs(f8[7:8].cpu().numpy() - e7).max())
    assert err7 <= 1e-3, err7
    util.check_float64("config3 b8 pair 7", f8[7:8], [p[7:8] for p in pyr8], util.float64_flows(w, True, im0[7:8], im1[7:8]),
                       F64_BOUND_PX["config3"])


def test_config4_960x1920_vs_oracle(pa):
    """configs[4] frame size (KITTI-shaped): odd-sized coarse levels 15x30 / 30x60."""
    net, w = make_net(pa, False)
    im0, im1 = util.smooth_images(2, 960, 1920, seed=43, shift=(-6, 4))
    final, pyr = net(gpu(im0), gpu(im1))
    assert final.shape == (2, 960, 1920, 2)
    assert [tuple(p.shape[1:3]) for p in pyr] == [(15, 30), (30, 60), (60, 120), (120, 240), (240, 480)]
    e_final, e_pyr = orc.OraclePWCDCNet(w)(im0[1:2], im1[1:2])
    err = float(np.abs(final[1:2].cpu().numpy() - e_final).max())
    assert err <= 1e-3, err
    for p, e in zip(pyr, e_pyr):
        assert float(np.abs(p[1:2].cpu().numpy() - e).max()) <= 5e-5
    util.check_float64("config4 pair 1", final[1:2], [p[1:2] for p in pyr], util.float64_flows(w, False, im0[1:2], im1[1:2]),
                       F64_BOUND_PX["config4"])


def test_config4_per_gpu_batch8_960x1920_pairs_vs_oracle(pa):
    """configs[4] at its real per-GPU workload: 16 pairs on 2 GPUs = 8 x 960x1920 per rank -- the tile plans,
    Winograd NT / split choices and cost-volume segmentations of N = 8, not those of N = 2.  Pairs 0 and 7
    against the oracle run on those pairs."""
    net, w = make_net(pa, False)
    im0, im1 = util.smooth_images(8, 960, 1920, seed=44, shift=(3, -5))
    final, pyr = net(gpu(im0), gpu(im1))
    assert final.shape == (8, 960, 1920, 2)
    onet = orc.OraclePWCDCNet(w)
    for i in (0, 7):
        e_final, e_pyr = onet(im0[i:i + 1], im1[i:i + 1])
        err = float(np.abs(final[i:i + 1].cpu().numpy() - e_final).max())
        assert err <= 1e-3, (i, err)
        for p, e in zip(pyr, e_pyr):
            assert float(np.abs(p[i:i + 1].cpu().numpy() - e).max()) <= 5e-5
        util.check_float64(f"config4_b8 pair {i}", final[i:i + 1], [p[i:i + 1] for p in pyr],
                           util.float64_flows(w, False, im0[i:i + 1], im1[i:i + 1]), F64_BOUND_PX["config4_b8"])


# ------------------------------------------------------------------ output ownership
def test_outputs_are_fresh_tensors_by_default(pa):
    """sess.run hands back new arrays on every call (reference test.py:51,55): a result held
    across a later forward must not change."""
    net, _ = make_net(pa, False)
    x0, x1 = util.smooth_images(2, 64, 128, seed=51)
    y0, y1 = util.smooth_images(2, 64, 128, seed=52, shift=(-2, 3))
    a, pyr_a, feats_a = net(gpu(x0), gpu(x1), with_features=True)      # recording call
    a_ref, pyr_ref, feats_ref = a.clone(), [p.clone() for p in pyr_a], [f.clone() for f in feats_a]
    b, pyr_b, feats_b = net(gpu(y0), gpu(y1), with_features=True)      # first replay, OTHER inputs
    torch.cuda.synchronize()
    # the recording call's results (pyramid_0 included: slices of plan-owned activations in the plan)
    # must have survived a replay that overwrote every plan buffer with other values
    assert torch.equal(a, a_ref) and all(torch.equal(p, q) for p, q in zip(pyr_a, pyr_ref))
    assert all(torch.equal(p, q) for p, q in zip(feats_a, feats_ref))
    assert not any(torch.equal(p, q) for p, q in zip(feats_a, feats_b))
    feats_b_ref = [f.clone() for f in feats_b]
    c, pyr_c, feats_c = net(gpu(x0), gpu(x1), with_features=True)      # second replay
    torch.cuda.synchronize()
    assert torch.equal(a, a_ref) and all(torch.equal(p, q) for p, q in zip(pyr_a, pyr_ref))
    assert all(torch.equal(p, q) for p, q in zip(feats_a, feats_ref))
    assert all(torch.equal(p, q) for p, q in zip(feats_b, feats_b_ref))
    assert not torch.equal(a, b)
    assert torch.equal(c, a) and all(torch.equal(p, q) for p, q in zip(pyr_c, pyr_a))
    assert all(torch.equal(p, q) for p, q in zip(feats_c, feats_a))
    ptrs = {t.data_ptr() for t in (a, b, c)}
    assert len(ptrs) == 3


def test_persistent_outputs_opt_in_aliases(pa):
    net, _ = make_net(pa, False, persistent_outputs=True)
    x0, x1 = util.smooth_images(1, 64, 128, seed=53)
    y0, y1 = util.smooth_images(1, 64, 128, seed=54, shift=(1, 1))
    a, _ = net(gpu(x0), gpu(x1))
    a_ref = a.clone()
    b, _ = net(gpu(y0), gpu(y1))
    assert b.data_ptr() == a.data_ptr() and not torch.equal(a, a_ref)   # overwritten, as documented


def test_plans_are_per_stream_and_bounded(pa):
    """Two forwards of one shape on different streams own different buffers (no race), and the
    number of kept plans is bounded (LRU).  (streams=1: the sub-batch mode keeps one plan more, by design.)"""
    net, _ = make_net(pa, False, max_plans=2, streams=1)
    x0, x1 = util.smooth_images(2, 64, 128, seed=55)
    y0, y1 = util.smooth_images(2, 64, 128, seed=56, shift=(2, -1))
    gx0, gx1, gy0, gy1 = gpu(x0), gpu(x1), gpu(y0), gpu(y1)
    ref_x, _ = net(gx0, gx1)
    ref_y, _ = net(gy0, gy1)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for _ in range(3):                      # record on each stream, then replay concurrently
        with torch.cuda.stream(s1):
            ox, _ = net(gx0, gx1)
        with torch.cuda.stream(s2):
            oy, _ = net(gy0, gy1)
        outs.append((ox, oy))
    torch.cuda.synchronize()
    for ox, oy in outs:
        assert torch.equal(ox, ref_x) and torch.equal(oy, ref_y)
    assert len(net._plans) <= 2
    bufs = [id(p.buffers) for p in net._plans.values()]
    assert len(set(bufs)) == len(bufs)
    for shape in ((1, 64, 64), (1, 64, 192), (1, 128, 128)):
        im = util.images(shape[0], shape[1], shape[2], seed=57)
        net(gpu(im[0]), gpu(im[1]))
    assert len(net._plans) <= 2


def test_load_weights_strict(pa):
    w = util.model_weights(False)
    net = pa.PWCDCNet()
    with pytest.raises(ValueError, match="missing"):
        net.load_weights({k: v for k, v in w.items() if "optflow_3" not in k})
    with pytest.raises(ValueError, match="unexpected"):
        net.load_weights(dict(w, **{"pwcdcnet/optflow_5/conv2d/kernel": np.zeros((3, 3, 4, 4), np.float32)}))
    with pytest.raises(ValueError, match="missing|unexpected|shape"):
        pa.PWCDCNet(use_dc=True).load_weights(w)            # non-DC checkpoint into a DC model
    bad = dict(w)
    k = "pwcdcnet/context/conv2d/kernel"
    bad[k] = np.zeros((3, 3, 35, 128), np.float32)
    with pytest.raises(ValueError, match="shape"):
        net.load_weights(bad)
    net.load_weights({k: w[k]}, strict=False)               # partial set, explicitly allowed
    net.load_weights(w)


# ------------------------------------------------------------------ bench.py launch
def _run_bench(extra, timeout=900):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1",
                          "--batch", "2", "--height", "128", "--width", "192", "--cpu-seconds", "1"] + extra,
                         capture_output=True, text=True, timeout=timeout)
    return out


def test_bench_spawns_its_ranks_with_rccl(pa):
    """`bench.py --gpus 1 --spawn`: the self-launch path the driver's `--gpus N` takes -- one
    torch.distributed.run rank per GPU, nccl (= RCCL) process group, stats all-gathered on
    device tensors."""
    out = _run_bench(["--gpus", "1", "--spawn"])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["config"]["global_batch"] == 2 and d["config"]["per_gpu_batch"] == 2
    assert "RCCL" in d["config"]["parallelism"]
    assert d["roofline"]["frac"] <= 1.0 and d["roofline_hbm"]["frac"] <= 1.0
    assert d["parity"]["max_abs_flows_final"] <= d["parity"]["tolerance"]


def test_bench_two_ranks_on_one_gpu(pa):
    """`bench.py --gpus 2 --share-gpu`: the N > 1 branch of the bench on a 1-GPU box -- two
    torch.distributed.run ranks that share device 0 and gather their statistics over gloo (RCCL refuses two ranks on one
    device): barriers on both sides of the timed region, a ForwardPipeline per rank, per-rank timings, value = all pairs over
    the slowest rank, the one-stream loop / op-level leg / parity on rank 0 only, one JSON line."""
    out = _run_bench(["--gpus", "2", "--share-gpu"])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 4 and d["config"]["per_gpu_batch"] == 2
    assert len(d["per_rank_ms_per_step"]) == 2 and d["scaling"] == "weak"
    assert abs(d["ms_per_step"] - max(d["per_rank_ms_per_step"])) <= 1e-9 * d["ms_per_step"]
    assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert "SHARE GPUs" in d["config"]["parallelism"] and "dp2" in d["config"]["parallelism"]
    assert d["range_status"]["flags"] == 0 and d["roofline"]["frac"] <= 1.0 and d["value_one_stream"] > 0
    assert "cpu_baseline" not in d and "parity" not in d          # (rank 0 at N = 1 only, by the contract)


def test_bench_train_mode_through_the_rccl_launch(pa):
    """`bench.py --mode train --gpus 1 --spawn`: training steps under torch.distributed.run -- the gradient all-reduce
    runs on the nccl (= RCCL) process group (world 1), the loss falls on the repeated batch."""
    out = _run_bench(["--gpus", "1", "--spawn", "--mode", "train", "--steps", "4"])
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("training_image_pairs_per_sec") and d["n_gpus"] == 1 and d["value"] > 0
    assert "all-reduce" in d["config"]["parallelism"]
    assert d["loss_last_step"] < d["loss_first_step"]


def test_bench_rejects_a_world_size_that_contradicts_gpus(pa):
    """--gpus must never be silently ignored."""
    more = torch.cuda.device_count() + 1
    out = _run_bench(["--gpus", str(more)])
    assert out.returncode != 0 and "GPU(s) are visible" in (out.stderr + out.stdout)
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29655")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "WORLD_SIZE" in (out.stderr + out.stdout)


def test_sub_batches_on_side_streams_give_the_same_flows(pa):
    """PWCDCNet(streams=2): the batch runs as two sub-batches on side HIP streams (their kernels overlap).  Same flows as
    the single-stream model, fresh tensors on every call, correct when calls follow each other without a sync."""
    w = util.model_weights(False, gain=1.2)
    im0, im1 = util.smooth_images(4, 128, 192, seed=93, shift=(2, -1))
    jm0, jm1 = util.smooth_images(4, 128, 192, seed=94, shift=(-3, 2))
    ref = pa.PWCDCNet()
    ref.load_weights(w)
    net = pa.PWCDCNet(streams=2)
    net.load_weights(w)
    g0, g1, h0, h1 = gpu(im0), gpu(im1), gpu(jm0), gpu(jm1)
    ra, rpa = ref(g0, g1)
    rb, _ = ref(h0, h1)
    for _ in range(3):                                  # recording call, then replays; back-to-back without syncs
        a, pyr_a = net(g0, g1)
        b, _ = net(h0, h1)
    assert a.data_ptr() != b.data_ptr()
    assert float((a - ra).abs().max()) <= 2e-5 * max(1.0, float(ra.abs().max()))
    assert float((b - rb).abs().max()) <= 2e-5 * max(1.0, float(rb.abs().max()))
    for x, y in zip(pyr_a, rpa):
        assert x.shape == y.shape and float((x - y).abs().max()) <= 2e-5 * max(1.0, float(y.abs().max()))
    # an odd batch falls back to the single-stream path
    c, _ = net(g0[:3], g1[:3])
    assert float((c - ra[:3]).abs().max()) <= 2e-5 * max(1.0, float(ra.abs().max()))
    # called on a stream of the caller's: sub-batch 0 runs on THAT stream, the results are ordered after it
    import torch
    user = torch.cuda.Stream()
    user.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(user):
        for _ in range(2):
            d, _ = net(h0, h1)
        d2 = d * 1.0                                    # consumer on the caller's stream
    user.synchronize()
    assert float((d2 - rb).abs().max()) <= 2e-5 * max(1.0, float(rb.abs().max()))
    side = [s for v in net._side_streams.values() if v for s in v]
    assert all(s.cuda_stream != user.cuda_stream for s in side) and len(net._side_streams) == 2
    # the placement verdict is visible
    rep = net.side_stream_report
    assert rep is not None and rep["verdict"] in ("vetted",) or "single stream" in rep["verdict"]
    assert net.effective_streams(g0.shape) == 2 and net.effective_streams(g0[:3].shape) == 1


def test_first_call_on_side_streams_is_already_right(pa):
    """the per-module weight caches are filled by whichever stream launches a layer first.  The first call of a
    shape therefore runs sub-batch 0 alone on the caller's stream before the side streams start; its result -- taken from a
    caller's stream that already has a backlog -- equals the single-stream model's."""
    import torch
    w = util.model_weights(False, gain=1.2)
    im0, im1 = util.smooth_images(4, 128, 192, seed=95, shift=(1, 2))
    g0, g1 = gpu(im0), gpu(im1)
    ref = pa.PWCDCNet(streams=1)
    ref.load_weights(w)
    r, rp = ref(g0, g1)
    torch.cuda.synchronize()
    for trial in range(3):
        net = pa.PWCDCNet(streams=2)
        net.load_weights(w)
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(6):                               # a backlog on the caller's stream: both sub-batches would start together
            big = big @ big * 1e-3
        a, pa_ = net(g0, g1)                             # FIRST call: packs every layer's weights
        torch.cuda.synchronize()
        assert float((a - r).abs().max()) <= 2e-5 * max(1.0, float(r.abs().max())), trial
        for x, y in zip(pa_, rp):
            assert float((x - y).abs().max()) <= 2e-5 * max(1.0, float(y.abs().max()))


def test_side_stream_probe_with_busy_dummy_streams(pa):
    """HIP maps streams onto a few hardware queues; a side stream behind the caller's queue costs 25 %.
    With 1 .. 4 dummy streams created AND used beforehand (the `used_dummies` cases of profiles/r03_exp_side_stream_queues.txt)
    the device-timed probe must still pick a stream on a queue of its own -- or fall back to one stream: the forward stays
    within 8 % of the clean placement either way, never at the 1.25x of a bad one."""
    import time
    import torch
    w = util.model_weights(False)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    im0 = torch.rand((8, 448, 1024, 3), generator=g, device="cuda")
    im1 = torch.rand((8, 448, 1024, 3), generator=g, device="cuda")

    def ms_per_forward(net, steps=12):
        for _ in range(4):
            net(im0, im1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            net(im0, im1)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps

    clean = pa.PWCDCNet(streams=2)                       # (one stream is the default since round 5: the probe only runs on request)
    clean.load_weights(w)
    base = ms_per_forward(clean)
    single = pa.PWCDCNet(streams=1)
    single.load_weights(w)
    one = ms_per_forward(single)
    assert clean.side_stream_report is not None
    worst = 0.0
    for ndummy in (1, 2, 3, 4):
        dummies = [torch.cuda.Stream() for _ in range(ndummy)]
        junk = torch.zeros(1024, device="cuda")
        for d in dummies:
            with torch.cuda.stream(d):
                junk.add_(1)
        torch.cuda.synchronize()
        net = pa.PWCDCNet(streams=2)
        net.load_weights(w)
        t = ms_per_forward(net)
        rep = net.side_stream_report
        assert rep is not None and (rep["verdict"] == "vetted" or "single stream" in rep["verdict"]), rep
        worst = max(worst, t)
        bound = (base if rep["verdict"] == "vetted" else one) * 1.08
        assert t <= bound, (ndummy, t, base, one, rep)
    assert worst <= 1.08 * max(base, one)
