"""N > 1 path on CPU: two processes over gloo run the same tile split + gather + de-interleave that
bench.py runs over RCCL, with the per-rank tiles rendered by the CPU oracle (no GPU here)."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = Path(__file__).resolve().parent.parent


def _worker(rank, world, port, w, h, strip, out_path):
    sys.path.insert(0, str(REPO))
    sys.path.insert(0, str(REPO / "sycl-ray-tracer_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle as O
    from rtamd import scenes
    from rtamd.dist import FrameGatherer
    sd = scenes.cube_scene()
    sc = O.OracleScene(sd)
    cam = O.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    f, _, rays = sc.render(cam, 1, 6, 2, nthreads=2, rank=rank, world=world, strip_rows=strip)
    fg = FrameGatherer(rank, world, w, h, strip, torch.device("cpu"))
    assert fg.rows == f.shape[0]
    fg.local[: fg.rows] = torch.from_numpy(f)
    frame = fg.gather()
    tot = torch.tensor([float(rays)], dtype=torch.float64)
    dist.all_reduce(tot, op=dist.ReduceOp.SUM)
    if rank == 0:
        np.savez(out_path, frame=frame.numpy(), rays=tot.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,h,strip", [(2, 45, 8), (3, 64, 8)])
def test_two_process_tile_gather_equals_single_frame(tmp_path, oracle, world, h, strip):
    from rtamd import scenes
    w = 48
    out = tmp_path / "frame.npz"
    port = 29500 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, w, h, strip, str(out)), nprocs=world, join=True)
    got = np.load(out)
    sd = scenes.cube_scene()
    sc = oracle.OracleScene(sd)
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    full, _, rays = sc.render(cam, 1, 6, 2)
    np.testing.assert_array_equal(got["frame"], full)
    assert int(got["rays"][0]) == rays


def test_strip_ownership_partitions_the_frame():
    from rtamd.dist import max_local_rows, strip_rows_of
    for h in (1, 7, 8, 9, 1080, 2160, 93):
        for world in (1, 2, 3, 4, 8):
            rows = [strip_rows_of(r, world, h, 8) for r in range(world)]
            assert sorted(sum(rows, [])) == list(range(h))
            assert max(len(r) for r in rows) == max_local_rows(world, h, 8)
    # 1080p over 8 GPUs: 135 strips -> 17 or 16 strips per rank
    assert sorted({len(strip_rows_of(r, 8, 1080)) for r in range(8)}) == [128, 136]


def _bench(args, env_extra=None, timeout=240):
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(REPO / "bench.py")] + [str(a) for a in args], cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("world", [2, 3])
def test_bench_launches_its_own_ranks(tmp_path, oracle, world):
    """`python bench.py --gpus N` with no launcher around it (no WORLD_SIZE): it must start its N ranks itself (a torch.distributed.run
    child process), run the multi-rank path — process group, all-reduces, gather, de-interleave — and print the one JSON line with the
    per-rank fields. Rehearsed on the CPU: backend gloo, the ranks' tiles rendered beforehand by the oracle and read from files
    (bench.py itself has no CPU renderer); the frame rank 0 assembled must be the oracle's full frame."""
    import json
    from rtamd import scenes
    w, h, strip = 64, 45, 8
    sd = scenes.cornell_scene()
    sc = oracle.OracleScene(sd)
    cam = oracle.camera(w, h, sd.camera.position, sd.camera.direction, sd.camera.focal_length)
    for rank in range(world):
        f, _, _ = sc.render(cam, 1, 4, 2, rank=rank, world=world, strip_rows=strip)
        np.save(tmp_path / f"tile_{rank}.npy", f)
    full, _, _ = sc.render(cam, 1, 4, 2)
    out = tmp_path / "frame.npy"
    dump = tmp_path / "outputs"
    p = _bench(["--gpus", world, "--steps", 3, "--warmup", 1, "--width", w, "--height", h, "--backend", "gloo", "--rehearsal-tiles", tmp_path, "--dump-frame", out,
                "--dump-outputs", dump, "--detail", 1])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    assert [ln for ln in p.stdout.splitlines() if ln.strip()] == lines, "stdout carries the JSON line and nothing else:\n" + p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["rccl_ranks"] == world and d["backend"] == "gloo" and d["steps"] == 3 and d["warmup"] == 1
    assert len(d["per_rank_ms"]) == world and all(ms > 0 for ms in d["per_rank_ms"]) and d["gather_ms"] > 0
    assert d["scaling"] == "strong" and d["ms_per_step"] > 0
    # the shared-scene path: generated once by rank 0, read from its file by the others — every rank holds the same bytes, and every rank
    # reports what its setup cost before the timed region
    assert len(d["scene_digests"]) == world and len(set(d["scene_digests"])) == 1, d["scene_digests"]
    assert len(d["setup_s_per_rank"]) == world and all(r["scene_s"] > 0 for r in d["setup_s_per_rank"])
    # (3 frames through 3 strip buffers with the exchange of frame i overlapping frame i + 1: the last frame's gather is the dumped one)
    np.testing.assert_array_equal(np.load(out), full)
    # --dump-outputs: the same frame as float32 (small enough to be whole) and the rays of the last frame over all ranks (none: tiles from
    # files); the unorm8 image stays on the ranks
    assert sorted(f.name for f in dump.iterdir()) == ["rehearsal_rays.npy", "rehearsal_rgba_f32.npy"]
    f32, rays = np.load(dump / "rehearsal_rgba_f32.npy"), np.load(dump / "rehearsal_rays.npy")
    assert f32.dtype == np.float32 and rays.dtype == np.float64
    np.testing.assert_array_equal(f32, full)
    np.testing.assert_array_equal(rays, [0.0])


def test_bench_dump_outputs_stay_within_their_budget(tmp_path):
    """--dump-outputs writes float32 / float64 only and at most 64 MB in all: frames too large together are cut to one seeded sample of
    pixels, the same for every renderer and every run; `--steps` below one is refused (ms_per_step divides by it)."""
    sys.path.insert(0, str(REPO))
    import bench
    h, w = 1080, 1920
    rng = np.random.default_rng(5)
    frame = rng.random((h, w, 4), dtype=np.float32)
    image = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    outputs = {name: {"rgba_f32": frame, "rgba_u8": image, "rays": np.array([1e9 + 1.0])} for name in bench.RENDERERS}
    for run in ("a", "b"):
        bench.write_outputs(tmp_path / run, outputs)
    files = sorted((tmp_path / "a").iterdir())
    assert sum(f.stat().st_size for f in files) <= bench.DUMP_BYTES
    index = np.load(tmp_path / "a" / "pixel_index.npy")
    assert index.dtype == np.float64 and index.size == bench.DUMP_SAMPLE_PIXELS and (np.diff(index) > 0).all() and index[-1] < h * w
    pix = index.astype(np.int64)
    for name in bench.RENDERERS:
        f32, u8 = np.load(tmp_path / "a" / f"{name}_rgba_f32.npy"), np.load(tmp_path / "a" / f"{name}_rgba_u8.npy")
        assert f32.dtype == u8.dtype == np.float32
        np.testing.assert_array_equal(f32, frame.reshape(-1, 4)[pix])
        np.testing.assert_array_equal(u8, image.reshape(-1, 4)[pix])
        assert np.load(tmp_path / "a" / f"{name}_rays.npy").tolist() == [1e9 + 1.0]
    for f in files:  # the same arguments, the same files
        assert (tmp_path / "b" / f.name).read_bytes() == f.read_bytes()
    small = {"megakernel": {"rgba_f32": frame[:36, :64], "rgba_u8": image[:36, :64], "rays": np.array([7.0])}}
    bench.write_outputs(tmp_path / "small", small)  # whole frames where they fit
    np.testing.assert_array_equal(np.load(tmp_path / "small" / "megakernel_rgba_f32.npy"), frame[:36, :64])
    assert not (tmp_path / "small" / "pixel_index.npy").exists()
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    assert bench.parse_args(["--steps", "7"]).steps == 7


def test_bench_full_legs_are_opt_in():
    """A plain run measures what the headline needs; `--full` adds the legs after the timed regions. Options that only feed those legs are
    refused without it, and a plain run's per-bounce rooflines say that their launch durations were not measured instead of reporting zeros."""
    sys.path.insert(0, str(REPO))
    import bench
    assert not bench.parse_args([]).full and bench.parse_args(["--full"]).full
    for only_full in (["--dump-pmc", "pmc.json"], ["--pipelined-renderer", "megakernel"]):
        with pytest.raises(SystemExit):
            bench.parse_args(only_full)
        assert bench.parse_args(["--full"] + only_full).full
    steps, rays = 4, 4_000_000
    for name in ("wavefront_per_bounce", "wavefront_per_bounce_fused"):
        plain = {"rays": rays * steps, "hot_ms": 0.0, "hot_launches": 0, "kernel_ms": {}, "kernels": {"wf_shade": 640 * steps}, "lanes": 3}
        roof = bench.roofline_of(name, bench.parse_args(["--steps", str(steps)]), plain, 1080, 1920, rays * steps, 0.5, steps)
        assert roof["achieved"] > 0 and roof["per_launch"]["achieved"] is None and "--full" in roof["per_launch"]["note"]
        full = dict(plain, hot_ms=50.0, hot_launches=640, kernel_ms={"wf_extend": 50.0, "wf_shade": 30.0}, kernels={"wf_shade": 640 * steps}, profiled_rays=rays)
        roof_full = bench.roofline_of(name, bench.parse_args(["--steps", str(steps), "--full"]), full, 1080, 1920, rays * steps, 0.5, 1)
        assert roof_full["achieved"] == roof["achieved"] and roof_full["per_launch"]["achieved"] > 0
        if name == "wavefront_per_bounce":
            assert roof["pipeline"]["k_wf_shade"]["mean_launch_ms"] is None and roof["pipeline"]["k_wf_extend"]["sum_launch_ms_per_frame"] is None
            assert roof["pipeline"]["launch_pairs_per_frame"] == roof_full["pipeline"]["launch_pairs_per_frame"] == 640
            assert roof_full["pipeline"]["k_wf_shade"]["mean_launch_ms"] > 0


def test_bench_launcher_reports_a_failing_rank(tmp_path):
    """A rank that fails (here: its tile file is missing) must make `bench.py --gpus N` exit non-zero, not hang and not print a line."""
    np.save(tmp_path / "tile_0.npy", np.zeros((24, 16, 4), np.float32))  # tile_1.npy is missing
    p = _bench(["--gpus", 2, "--steps", 1, "--warmup", 0, "--width", 16, "--height", 40, "--backend", "gloo", "--rehearsal-tiles", tmp_path], timeout=300)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]


def test_bench_refuses_a_cpu_backend_without_tiles():
    p = _bench(["--gpus", 1, "--backend", "gloo"])
    assert p.returncode != 0 and "rehearsal" in (p.stdout + p.stderr)
