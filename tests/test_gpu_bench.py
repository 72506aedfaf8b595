"""bench.py's plain run and --dump-outputs on one GPU (the default workload, C2).

A plain run (`--gpus 1 --steps N --warmup W`) times N headline steps and
prints one line without the legs and per-kernel figures of --full (those are
exercised by test_gpu_rccl.py and test_distributed.py).  --dump-outputs
writes what the last timed wc_forward produced: every unit's kept count and
payload offset, and the decoded payloads of a fixed sample of units, which
must be the oracle's payloads of the same cells."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
KEEP = float(np.float32(0.999))
FULL_ONLY = ("stage_ms_per_launch", "roofline", "roofline_path", "inverse", "host", "c3", "f32_64", "c5", "c4")


def test_legs_without_full_is_an_argument_error(tmp_path):
    """--legs selects among what --full runs; alone it is refused, not ignored."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--legs", "c5"], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and "--legs needs --full" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(dump)], env=env, capture_output=True, text=True, timeout=110,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "cells/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0
    # value is the batch's cells over one timed step
    assert out["value"] == pytest.approx(1024 * 64 ** 3 / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in out] and out["cpu_baseline"] is None

    files = {p.stem: np.load(p) for p in dump.glob("*.npy")}
    assert sorted(files) == ["kept", "offsets", "payload_header", "payload_runs", "payload_vals", "sample_units"]
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64e6
    kept, offs = files["kept"].astype(np.int64), files["offsets"].astype(np.int64)
    assert kept.shape == (1024,) and offs.shape == (1025,)
    # wc_forward's fixed slots (include/wavelet_amd.h): the worst-case sizes 24 + 8*W*H*D of the
    # units before, starting at 4; offsets[n] is the end of the last unit's bytes
    assert np.array_equal(offs[:1024], 4 + np.arange(1024) * (24 + 8 * 64 ** 3))
    assert offs[1024] == offs[1023] + 20 + 8 * kept[1023]
    assert np.all((kept > 0) & (kept <= 64 ** 3))
    assert int(kept.sum()) == round(out["kept_fraction"] * 1024 * 64 ** 3)
    sample = files["sample_units"].astype(np.int64)
    hdr = files["payload_header"].astype(np.int64)
    assert len(sample) >= 8 and len(set(sample.tolist())) == len(sample) and hdr.shape == (len(sample), 5)
    assert np.array_equal(hdr[:, 4], kept[sample]) and np.all(hdr[:, :4] == [64, 64, 64, 64 ** 3])
    assert files["payload_runs"].shape == files["payload_vals"].shape == (int(kept[sample].sum()),)
    assert files["payload_vals"].dtype == np.float32

    # the first and the last sampled unit's pairs are the oracle's for the same cells
    import torch
    import bench_workloads as bw
    units = bw.WORKLOADS["c2"]["units"]()
    start = np.concatenate([[0], np.cumsum(kept[sample])])
    for j in (0, len(sample) - 1):
        u = units[int(sample[j])]
        cells, _, _ = bw.synth_cells(torch, torch.device("cuda", 0), [u], "f64")
        box = cells[:u.cells].cpu().numpy().reshape(u.D, u.H, u.W)
        want, wk = oracle.compress_payload(oracle.narrow(box), KEEP)
        _, _, runs, vals = oracle.parse_payload(want)
        assert wk == kept[sample[j]]
        a, b = int(start[j]), int(start[j + 1])
        assert np.array_equal(files["payload_runs"][a:b], runs.astype(np.float64))
        assert files["payload_vals"][a:b].tobytes() == vals.tobytes()
