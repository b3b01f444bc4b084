"""CPU: the process-launching half of bench.py (`--gpus N` without a launcher around it).  No GPU here, so the ranks
themselves stop at "no GPU, no number" -- what is checked is that N of them are started with the right environment,
that their failure is the parent's exit code, and that a mislabelled run is refused."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(kw)
    return env


def test_world_size_must_match_gpus():
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=120,
                         env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert out.returncode != 0 and "WORLD_SIZE=1" in out.stderr and not out.stdout.strip()


def test_parent_starts_n_ranks_and_reports_their_failure():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("with a GPU the ranks run for real: tests/test_bench_contract_gpu.py")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1"], capture_output=True,
                         text=True, timeout=300, env=_env(GI2D_BENCH_BACKEND="gloo"))
    assert out.returncode != 0
    assert out.stderr.count("no GPU, no number") == 2, out.stderr[-1500:]  # both ranks got as far as the device check
    assert "rank exit codes" in out.stderr and not out.stdout.strip()


def test_launch_ranks_sets_the_rendezvous_environment(tmp_path, monkeypatch):
    """launch_ranks() with a stand-in for the interpreter: every rank must see its own RANK / LOCAL_RANK, the common
    WORLD_SIZE / MASTER_ADDR / MASTER_PORT, and the original argument list."""
    sys.path.insert(0, ROOT)
    import bench
    probe = tmp_path / "probe.sh"
    probe.write_text("#!/bin/sh\necho \"$RANK $LOCAL_RANK $WORLD_SIZE $MASTER_ADDR $MASTER_PORT $HSA_ENABLE_IPC_MODE_LEGACY $*\" "
                     f">> {tmp_path}/seen.txt\n[ \"$RANK\" = 0 ] && echo '{{\"n_gpus\": 3}}'\nexit 0\n")
    probe.chmod(0o755)
    monkeypatch.setattr(bench.sys, "executable", str(probe))
    monkeypatch.delenv("MASTER_PORT", raising=False)
    rc = bench.launch_ranks(3, ["--gpus", "3", "--steps", "5"])
    assert rc == 0
    rows = sorted(l.split() for l in (tmp_path / "seen.txt").read_text().splitlines())
    assert [r[0] for r in rows] == ["0", "1", "2"] and [r[1] for r in rows] == ["0", "1", "2"]
    assert all(r[2] == "3" and r[3] == "127.0.0.1" and r[5] == "0" for r in rows)
    assert len({r[4] for r in rows}) == 1 and int(rows[0][4]) > 0
    assert all(r[-4:] == ["--gpus", "3", "--steps", "5"] for r in rows)


def test_full_is_off_by_default_and_the_optional_legs_ask_for_it(capsys):
    """A plain run measures the headline alone: --full is off unless given, the per-leg switches stay accepted without
    it, and the two legs that are off by default refuse to be asked for without it rather than be dropped in silence."""
    import pytest
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"]).full is False
    assert bench.parse(["--images", "0", "--no-cpu-baseline", "--no-batched", "--no-static", "--no-dropin"]).full is False
    args = bench.parse(["--full", "--train-step", "--images-per-gpu-probe"])
    assert args.full is True and args.train_step and args.images_per_gpu_probe
    for flag in ("--train-step", "--images-per-gpu-probe"):
        with pytest.raises(SystemExit) as e:
            bench.parse([flag])
        assert e.value.code == 2 and "--full" in capsys.readouterr().err


def test_stored_counters_exist_for_the_kernels_bench_names():
    """bench.py copies `roofline.traffic` (and the VALU counters) from profiles/traffic.json by KERNEL NAME; a kernel that
    gains a template argument silently turns the figure into null.  The names the default run, BASELINE config 4 and the
    24-image block use must have an entry with HBM bytes -- regenerate the profiles (tools/profile_rounds.sh,
    tools/make_profiles_rounds.py) when this fails."""
    sys.path.insert(0, ROOT)
    import bench
    cases = [("gi2d::fast_fwdbwd_kernel<1, 0, true>", 50000, 512, 768, None),
             ("gi2d::fast_fwdbwd_kernel<1, 1, false> + gi2d::fast_fwdbwd_kernel<1, 2, false>", 50000, 1356, 2040, None),
             ("gi2d::fast_fwdbwd_batched_kernel<1, 1> + gi2d::fast_fwdbwd_batched_kernel<1, 2>", 50000, 512, 768, 24)]
    for kernel, n, h, w, k in cases:
        traffic, source = bench.pmc_traffic(kernel, n, h, w, k)
        assert traffic and traffic > 1e6, (kernel, source)
        assert source.startswith("stored:"), source
    valu = bench.valu_roofline(cases[0][0], 50000, 512, 768, 18.0)
    assert valu.get("insts_per_image", 0) > 1e6, valu


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_above_the_limit(tmp_path):
    """dump_outputs(): one float32 / float64 .npy per array; above the byte limit every array shrinks to a sample of
    its elements that is the same from call to call, and the files stay under the limit."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(5)
    arrays = {"ids": np.arange(12, dtype=np.int32).reshape(3, 4), "img": rng.random((40, 60, 3)).astype(np.float32),
              "wide": rng.random((500, 2))}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["ids", "img", "wide"]
    assert got["ids"].dtype == np.float32 and got["img"].dtype == np.float32 and got["wide"].dtype == np.float64
    assert all(np.array_equal(got[k], arrays[k]) for k in arrays)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, suffix="_rank1", limit=9000)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["ids_rank1.npy", "img_rank1.npy", "wide_rank1.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= 9000
    for f in files:
        a, b = np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)
        full = arrays[f[:-len("_rank1.npy")]]
        assert a.ndim == 1 and 0 < a.size < full.size and np.array_equal(a, b)
        assert np.isin(a, full.astype(a.dtype)).all()
