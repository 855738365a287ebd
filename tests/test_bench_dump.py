"""bench.py --dump-outputs: what the timed path computed, written as .npy files so that two builds of the project can
be compared output for output.  The selection logic runs on the CPU; the end-to-end runs need the GPU (-m gpu)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import bench

CAP = 64 * 10**6  # bytes that one dump may write in all


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(entry.ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--pool-candidates", "1",
           "--no-cpu-baseline", "--no-ceiling", "--no-side-figures", "--dump-outputs", str(out_dir)] + list(extra)
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    return {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_dump_selection_is_whole_when_small_and_a_fixed_sample_under_the_cap_when_large():
    assert bench.dump_selection(3, 40, 96, 4) == ([0, 1, 2], list(range(40)))
    for F, h, w, bpp in [(256, 2160, 3840, 4), (256, 2160, 3840, 1), (512, 2160, 3840, 1), (2, 8192, 8192, 4)]:
        frames, rows = bench.dump_selection(F, h, w, bpp)
        assert frames == bench.sample_frame_ids(F)
        assert len(frames) * len(rows) * w * bpp * 4 <= bench.DUMP_BYTES < CAP
        assert rows == sorted(set(rows)) and {0, 1, 2, h - 3, h - 2, h - 1} <= set(rows)
        assert all(0 <= r < h for r in rows) and len(rows) > 6
        assert (frames, rows) == bench.dump_selection(F, h, w, bpp)  # fixed: same shape, same sample


def test_steps_below_one_is_an_argument_error():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse(["--steps", "7"]).steps == 7


@pytest.mark.gpu
def test_dump_is_the_timed_output_and_repeats_run_to_run(tmp_path, oracle):
    """A small Sobel batch fits whole: the dump equals the oracle on the same synthetic frames, and a second run with
    the same arguments writes the same arrays."""
    args = ("--filter", "sobel", "--frames", "3", "--width", "200", "--height", "61", "--synth-mode", "1")
    a = _bench(tmp_path / "a", *args)
    b = _bench(tmp_path / "b", *args)
    assert sorted(a) == ["output", "output_frames", "output_rows"]
    assert a["output"].dtype == np.float32 and a["output"].shape == (3, 61, 200)
    assert a["output_frames"].dtype == np.float64 and list(a["output_frames"]) == [0, 1, 2]
    frames = oracle.synth_rgba(200, 61, 3, first_frame=0, seed=0x5EED, mode=1)
    for f in range(3):
        assert np.array_equal(a["output"][f], oracle.sobel_rgba(frames[f]).astype(np.float32))
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
def test_dump_of_a_4k_batch_is_a_sample_under_the_cap(tmp_path, oracle):
    """The headline shape (4K Gaussian): a fixed sample of whole rows of the parity frames, within 1 LSB of the
    oracle like the frames themselves, and under 64 MB in all."""
    d = tmp_path / "dump"
    got = _bench(d, "--frames", "8")
    assert sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)) <= CAP
    frames, rows = bench.dump_selection(8, 2160, 3840, 4)
    assert list(got["output_frames"]) == frames and list(got["output_rows"]) == rows
    assert got["output"].shape == (len(frames), len(rows), 3840, 4)
    src = oracle.synth_rgba(3840, 2160, 8, first_frame=0, seed=0x5EED, mode=0)
    threads = max(1, min(oracle.max_threads(), 32))
    for i, f in enumerate(frames):
        ref = oracle.gauss_rgba(src[f], 5, 1.5, threads=threads)[rows].astype(np.float32)
        assert np.abs(got["output"][i] - ref).max() <= 1
