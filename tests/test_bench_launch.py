"""bench.py's own launch logic on the CPU tier: `python bench.py --gpus 2` with no launcher around it must start one rank per
"GPU" under torch.distributed.run itself (it used to measure one GPU and print n_gpus 1), run the replica line and (with --full) the
tile-sharded leg, and print ONE JSON line with n_gpus 2.  A plain run times exactly --steps steps once and, with --dump-outputs, writes
the frame its last step decoded.  The library here is the SIMT-interpreter build (M355_LIB), the picture a
256x192 one, the exchanges run over gloo: a plumbing check of the script, never a measurement."""
import json
import os
import subprocess
import sys

import numpy as np

from test_emu_picture import EMU_SO, emu_lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, env_extra=None):
    env = dict(os.environ, M355_LIB=EMU_SO, OMP_NUM_THREADS="1", M355_BENCH_SHARD_TIMEOUT="600")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny_4tiles", "--steps", "2", "--warmup", "1", "--repeats", "1", "--full",
           "--no-cpu-baseline", "--no-end-to-end", "--no-with-upload", "--no-dependent-chain"] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)


def test_bench_gpus_2_launches_itself(emu_lib):  # noqa: F811
    r = run_bench(["--gpus", "2"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "pictures/2" and d["scaling"] == "weak"
    ts = d["tile_sharded"]
    assert "error" not in ts, ts
    assert ts["frames_identical_on_all_ranks"] is True and ts["tiles_per_rank"] == 2.0 and ts["scaling"] == "strong"


def test_bench_gpus_mismatch_fails_loudly(emu_lib):  # noqa: F811
    r = run_bench(["--gpus", "2"], env_extra={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stdout + r.stderr)


FULL_ONLY = ("ms_per_step_one_in_flight", "stage_ms", "roofline", "verified", "rotating_references", "dependent_chain", "with_upload",
             "tile_sharded", "cpu_baseline", "end_to_end")


def test_bench_plain_run_dumps_the_last_frame(emu_lib, oracle, tmp_path):  # noqa: F811
    from libde265_amd import synth, worklist
    from oracle_py import Oracle
    env = dict(os.environ, M355_LIB=EMU_SO, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        out = tmp_path / ("out%d" % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "tiny_4tiles",
                            "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["metric"] == "decoded CTBs/s" and d["unit"] == "CTB64/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
        assert d["steps"] == 3 and d["repeats"] == 1 and d["ms_per_step"] > 0
        assert abs(d["value"] * d["ms_per_step"] / (1e3 * d["config"]["ctbs_per_picture"]) - 1) < 1e-9
        assert not [k for k in FULL_ONLY if k in d], d
        dumps.append([np.load(str(out / (n + ".npy"))) for n in ("y", "cb", "cr")])
    # what the oracle decodes from the same lists and reference planes
    cfg = dict(synth.CONFIGS["tiny_4tiles"])
    pic = synth.picture(**cfg)
    pp = pic.pp[0]
    geo = (int(pp["width"]), int(pp["height"]), int(pp["chroma_format_idc"]), int(pp["bit_depth_luma"]))
    o = Oracle(oracle)
    refs = {}
    for i in range(cfg["n_refs"]):
        refs[i] = o.frame_new(pp)
        o.frame_set_planes(refs[i], synth.ref_planes(cfg["seed"] + 17 * i, *geo))
    dst = o.frame_new(pp)
    pic.ref_frames = [i if i < len(refs) else -1 for i in range(worklist.MAX_REF_FRAMES)]
    assert o.decode(pic, dst, refs) == 0
    want = o.frame_planes(dst)
    for a, b, w in zip(dumps[0], dumps[1], want):
        assert a.dtype == np.float32 and a.shape == w.shape
        assert np.array_equal(a, b) and np.array_equal(a, w.astype(np.float32))


def test_bench_dump_samples_large_frames(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 1024, (64, 96), dtype=np.uint16), rng.integers(0, 1024, (32, 48), dtype=np.uint16),
              rng.integers(0, 1024, (32, 48), dtype=np.uint16)]
    bench.dump_outputs(str(tmp_path / "whole"), planes)                 # within the budget: the planes as they are
    for n, p in zip(("y", "cb", "cr"), planes):
        a = np.load(str(tmp_path / "whole" / (n + ".npy")))
        assert a.dtype == np.float32 and np.array_equal(a, p.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2000)
    got = []
    for k in range(2):
        bench.dump_outputs(str(tmp_path / ("s%d" % k)), planes)
        got.append([np.load(str(tmp_path / ("s%d" % k) / (n + ".npy"))) for n in ("y", "cb", "cr")])
    assert sum(a.size for a in got[0]) <= 2000
    for a, b, p in zip(got[0], got[1], planes):
        assert a.dtype == np.float32 and a.ndim == 1 and a.size == p.size * 2000 // sum(q.size for q in planes)
        assert np.array_equal(a, b)                                     # the same positions every run
        assert np.isin(a, p.astype(np.float32)).all()
