"""CPU, world_size 2 over gloo: the N > 1 path of bench.py.

1. the collective pieces: rank 0 owns the packed weight buffer, every other rank receives it by a chunked
   broadcast, utterances are sharded in contiguous blocks, the timing reduction takes the max over ranks;
2. bench.py's own control flow (`bench.run_bench`) with a CPU stand-in workload: finalize_distributed with
   materialize=False on rank 1, shard_range over the global batch, barrier-bracketed timing, rank 0's result line;
3. `python bench.py --gpus N` without a launcher starts its ranks as a child process and relays rank 0's line
   (checked with the launcher module replaced by a stub: there is no GPU in this container)."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _cpu_only_rank():
    """These ranks are CPU stand-ins and must not open the GPU.  dist.barrier() asks torch._C._get_accelerator()
    which device to use, and on a ROCm build that query counts devices, i.e. initialises HIP and opens the GPU in
    every rank -- eight of them beside a test process that already holds the device are more than a shared GPU host
    allows.  Answering "cpu" takes barrier()'s own CPU branch, which gloo runs anyway."""
    torch._C._get_accelerator = lambda: torch.device("cpu")


def _worker(rank, world, port, out):
    _cpu_only_rank()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from megatts2_hierspeechpp_amd import parallel
    r, lr, w = parallel.init_distributed("gloo")
    assert (r, w) == (rank, world)
    # the arena stand-in: rank 0 holds the packed weights, the others an empty layout
    n = (3 << 20) + 17
    buf = torch.arange(n, dtype=torch.float32) if rank == 0 else torch.zeros(n)
    parallel.broadcast_buffer(buf, src=0, chunk_elems=1 << 20)     # several chunks + a ragged tail
    ok = bool((buf == torch.arange(n, dtype=torch.float32)).all())
    lo, hi = parallel.shard_range(33, rank, world)
    tmax = parallel.barrier_max(1.0 + rank, torch.device("cpu"))
    every = parallel.gather_floats(10.0 * rank, torch.device("cpu"))
    out.put((rank, ok, (lo, hi), tmax, every))
    dist.destroy_process_group()


def test_broadcast_shard_and_timing_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _, _, _ in res)
    assert [span for _, _, span, _, _ in res] == [(0, 17), (17, 33)]
    assert all(t == 2.0 for _, _, _, t, _ in res)
    assert all(e == [0.0, 10.0] for *_, e in res)


# ------------------------------------------------------------------ bench.py's N = 2 control flow on CPU
class _Arena:
    def __init__(self, buffer):
        self.buffer = buffer


class _StandInModel(torch.nn.Module):
    """Same finalize() contract as the product models (hip_layers.finalize): every rank lays out an identical
    arena, only `materialize=True` fills it."""
    N = (1 << 18) + 5

    def finalize(self, device, materialize=True):
        buf = torch.zeros(self.N, dtype=torch.float32, device=device)
        if materialize:
            buf.copy_(torch.arange(self.N, dtype=torch.float32) % 251.0)
        self.arena = _Arena(buf)
        return self.arena


class _StandInWorkload:
    samples_per_utterance = 1000

    def __init__(self, args, rank, world, dev):
        self.model, self.rank, self.dev = _StandInModel(), rank, dev
        self.shard = None

    def prepare(self, lo, hi):
        self.shard = (lo, hi)
        self.x = torch.arange(lo, hi, dtype=torch.float32)

    def make_step(self):
        def step():
            # uses the broadcast weights: a rank that did not receive them fails check()
            return (self.x.sum() + self.model.arena.buffer.sum(),)
        return step

    def check(self, out):
        want = torch.arange(self.shard[0], self.shard[1], dtype=torch.float32).sum() + \
            (torch.arange(_StandInModel.N, dtype=torch.float32) % 251.0).sum()
        assert torch.equal(out[0], want), (self.rank, out[0], want)

    def describe(self, world):
        return {"workload": "cpu stand-in", "global_batch": 7 * world}


def _bench_worker(rank, world, port, out):
    _cpu_only_rank()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--gpus", str(world), "--steps", "3", "--warmup", "1", "--batch", "7"])
    result, wl = bench.run_bench(args, _StandInWorkload, backend="gloo", device=torch.device("cpu"))
    out.put((rank, result, wl.shard))
    dist.barrier()
    dist.destroy_process_group()


def test_bench_control_flow_world2_cpu_stand_in():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bench_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, line, shard0), (r1, none, shard1) = res
    assert none is None and line is not None            # only rank 0 reports
    assert shard0 == (0, 7) and shard1 == (7, 14)       # contiguous shards of the global batch 7 x 2
    assert line["n_gpus"] == 2 and line["rccl_world"] == 2 and line["scaling"] == "weak"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["config"]["shard_of_rank0"] == [0, 7]
    assert line["broadcast_ms"] > 0 and line["rank_ms_per_step"]["min"] <= line["rank_ms_per_step"]["max"]
    assert line["pack_ms"] > 0 and line["broadcast_gbs"] > 0       # the collective alone, apart from the packing
    # whole-job value: the units ALL ranks processed over the max-over-ranks time
    assert abs(line["value"] - 14 * 1000 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-6 * line["value"]
    json.dumps(line)


def _force_worker(port, out):
    _cpu_only_rank()
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import bench
    from megatts2_hierspeechpp_amd import parallel
    args = bench.parse_args(["--gpus", "1", "--force-dist", "--steps", "2", "--warmup", "1", "--batch", "5"])
    result, wl = bench.run_bench(args, _StandInWorkload, backend="gloo", device=torch.device("cpu"))
    out.put((result, wl.shard, parallel.collectives_on(), dist.is_initialized()))
    dist.destroy_process_group()


def test_force_dist_runs_the_collectives_at_world_size_1():
    """`--force-dist`: the one-rank job forms its process group and goes through the broadcast branch, the barriers and
    the timing reductions (the GPU twin of this test runs it over RCCL on the device)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_force_worker, args=(_free_port(), q))
    p.start()
    line, shard, coll, init = q.get(timeout=180)
    p.join(timeout=60)
    assert p.exitcode == 0 and coll and init and shard == (0, 5)
    assert line["rccl_world"] == 1 and line["backend"] == "gloo" and line["broadcast_ms"] > 0 and line["broadcast_gbs"] > 0


def _bench_worker8(rank, world, port, out, global_batch):
    _cpu_only_rank()
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    import bench
    argv = ["--gpus", str(world), "--steps", "2", "--warmup", "1", "--batch", "32"]
    if global_batch is not None:
        argv += ["--global-batch", str(global_batch)]
    args = bench.parse_args(argv)
    result, wl = bench.run_bench(args, _StandInWorkload, backend="gloo", device=torch.device("cpu"))
    out.put((rank, result, wl.shard))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("global_batch", [None, 250])
def test_bench_control_flow_world8_cpu_stand_in(global_batch):
    """BASELINE.json configs[4]'s shape -- 8 ranks, 256 utterances, 32 per rank -- through bench.run_bench on gloo
    (VERDICT r03 item 1b), and an uneven global batch of 250 (shards of 32 / 32 / 31 x 6): every rank's shard is
    contiguous, the shards tile the batch, `value` counts what ALL ranks processed."""
    world = 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bench_worker8, args=(r, world, port, q, global_batch)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    total = 256 if global_batch is None else global_batch
    shards = [sh for _, _, sh in res]
    assert shards[0][0] == 0 and shards[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(shards, shards[1:]))            # contiguous, no gap, no overlap
    sizes = [hi - lo for lo, hi in shards]
    assert max(sizes) - min(sizes) <= 1 and (sizes == [32] * 8 if global_batch is None else sizes == [32, 32] + [31] * 6)
    lines = [r for _, r, _ in res]
    assert lines[0] is not None and all(ln is None for ln in lines[1:])     # only rank 0 reports
    line = lines[0]
    # a fixed --global-batch is a strong-scaling run (the total work does not grow with the rank count); batch x gpus is weak
    assert line["n_gpus"] == 8 and line["rccl_world"] == 8 and line["backend"] == "gloo"
    assert line["scaling"] == ("weak" if global_batch is None else "strong")
    assert line["config"]["shard_of_rank0"] == [0, 32] and line["config"]["global_batch"] == total
    assert line["broadcast_ms"] > 0 and line["pack_ms"] > 0
    assert abs(line["value"] - total * 1000 * 2 / (line["ms_per_step"] * 2e-3)) < 1e-6 * line["value"]
    json.dumps(line)


def test_bench_gpus_n_starts_its_own_ranks(tmp_path):
    """WORLD_SIZE unset and --gpus 2: the parent starts `python -m torch.distributed.run ... bench.py` as a CHILD
    (before importing torch itself) and relays rank 0's line.  Here the child's `torch.distributed.run` is a stub
    package first on PYTHONPATH that records its argv and prints a result line."""
    fake = tmp_path / "torch" / "distributed"
    fake.mkdir(parents=True)
    (tmp_path / "torch" / "__init__.py").write_text("")
    (fake / "__init__.py").write_text("")
    (fake / "run.py").write_text(
        "import json, os, sys\n"
        "assert 'WORLD_SIZE' not in os.environ\n"
        "print('some launcher chatter')\n"
        "print(json.dumps({'metric': 'stub', 'argv': sys.argv[1:]}))\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = str(tmp_path)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout                      # exactly one JSON line on stdout
    argv = json.loads(lines[0])["argv"]
    assert "--nproc-per-node=2" in argv and "--nnodes=1" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1"
    assert argv[-4:] == ["--gpus", "2", "--steps", "4"] and argv[-5].endswith("bench.py")
    assert "some launcher chatter" in p.stderr            # everything else is relayed on stderr


# ------------------------------------------------------------------ bench.py --dump-outputs / --steps on CPU
class _CountingWorkload(_StandInWorkload):
    """Each call of the step returns a new value: what run_bench keeps must be the last timed step's output."""

    def make_step(self):
        self.calls = 0

        def step():
            self.calls += 1
            return (torch.full((2, 1, 6), float(self.calls)), torch.full((2, 1, 3), -float(self.calls)))
        return step

    def check(self, out):
        pass


def test_bench_steps_and_dump_outputs(tmp_path):
    """`--steps` is the number of timed steps (`ms_per_step` is their mean), the last timed step's outputs are what
    `--dump-outputs` writes, float32, and --steps below 1 is refused."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    args = bench.parse_args(["--gpus", "1", "--steps", "4", "--warmup", "2", "--batch", "2",
                             "--dump-outputs", str(tmp_path / "d")])
    result, wl = bench.run_bench(args, _CountingWorkload, backend="gloo", device=torch.device("cpu"))
    assert wl.calls == 2 + 4 and result["steps"] == 4 and result["ms_per_step"] > 0
    desc = bench.dump_outputs(wl.last_out, args.dump_outputs)
    audio, source = np.load(tmp_path / "d" / "audio.npy"), np.load(tmp_path / "d" / "source.npy")
    assert audio.dtype == np.float32 and audio.shape == (2, 1, 6) and (audio == 6.0).all()
    assert source.dtype == np.float32 and source.shape == (2, 1, 3) and (source == -6.0).all()
    assert desc["arrays"]["audio"]["shape"] == [2, 1, 6] and "sample" not in desc["arrays"]["audio"]
    json.dumps(desc)


def test_bench_dump_outputs_sample_is_bounded_and_fixed(tmp_path):
    """Outputs above the byte cap are cut to a seeded sample: under the cap in all, the same elements every run."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    out = (torch.arange(3000, dtype=torch.float32).view(3, 1, 1000), torch.arange(300, dtype=torch.float64).view(3, 1, 100))
    written = []
    for run in ("a", "b"):
        desc = bench.dump_outputs(out, str(tmp_path / run), max_bytes=4000)
        arrs = [np.load(tmp_path / run / f"{n}.npy") for n in bench.OUTPUT_NAMES]
        assert all(a.dtype == np.float32 for a in arrs) and sum(a.nbytes for a in arrs) <= 4000
        assert all("sample" in e for e in desc["arrays"].values())
        written.append(arrs)
    assert all(np.array_equal(x, y) for x, y in zip(*written))
    audio = written[0][0]
    assert len(audio) > 0 and np.all(np.diff(audio) > 0)       # sorted positions of the flat array, no repeats


# ------------------------------------------------------------------ bench.py: a plain run against --full
def test_bench_full_parts():
    """A plain run measures the headline alone; --full adds the roofline pass, and at N = 1 the CPU baseline and
    extra_configs, each of which its --no-* option still leaves out.  --dump-launches needs the roofline pass."""
    sys.path.insert(0, ROOT)
    import bench
    plain = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert not plain.full and bench.full_parts(plain, 1) == set()
    assert bench.full_parts(bench.parse_args(["--no-roofline", "--no-extra"]), 1) == set()
    full = bench.parse_args(["--full"])
    assert bench.full_parts(full, 1) == {"roofline", "cpu_baseline", "extra_configs"}
    assert bench.full_parts(full, 2) == {"roofline"}
    assert bench.full_parts(bench.parse_args(["--full", "--no-extra", "--no-cpu-baseline"]), 1) == {"roofline"}
    assert bench.full_parts(bench.parse_args(["--full", "--no-roofline"]), 1) == {"cpu_baseline", "extra_configs"}
    bench.parse_args(["--full", "--dump-launches", "t.txt"])
    for argv in (["--dump-launches", "t.txt"], ["--full", "--no-roofline", "--dump-launches", "t.txt"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)


@pytest.mark.parametrize("full", [False, True])
def test_bench_main_runs_only_what_is_asked(monkeypatch, capfd, tmp_path, full):
    """bench.main with the timed run stubbed out: a plain run goes from the timed steps to the dump and the line, and
    starts none of the --full passes; with --full (extra_configs left out) the roofline pass and the CPU baseline run,
    in that order, after the dump."""
    sys.path.insert(0, ROOT)
    import bench
    calls = []
    wl = _CountingWorkload(None, 0, 1, torch.device("cpu"))
    wl.last_out = (torch.zeros(2, 1, 6), torch.ones(2, 1, 3))

    def fake_run_bench(args, make_workload):
        calls.append("timed")
        return {"metric": bench.METRIC, "value": 1.0, "ms_per_step": 1.0, "n_gpus": 1}, wl

    monkeypatch.setattr(bench, "run_bench", fake_run_bench)
    monkeypatch.setattr(bench, "dump_outputs", lambda out, path: calls.append("dump") or {"dir": path})
    monkeypatch.setattr(bench, "vocoder_roofline",
                        lambda args, wl_, result: calls.append("roofline") or result.update(roofline={"frac": 0.5}))
    monkeypatch.setattr(bench, "cpu_baseline", lambda args, wl_, result: calls.append("cpu_baseline"))
    argv = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "d")]
    if full:
        argv += ["--full", "--no-extra"]
    saved = os.dup(1)                      # main() points descriptor 1 at stderr for the rest of the process
    try:
        assert bench.main(argv) == 0
    finally:
        os.dup2(saved, 1)
        os.close(saved)
    assert calls == (["timed", "dump", "roofline", "cpu_baseline"] if full else ["timed", "dump"])
    lines = [ln for ln in capfd.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["dump_outputs"]["dir"] == str(tmp_path / "d")
    assert ("roofline" in line) == full and "extra_configs" not in line
