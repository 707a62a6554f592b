"""bench.py --dump-outputs: what the last timed inference step returned, written as .npy files (float32 / float64, at most
64 MB in all) so that two builds can be compared output for output.  The CPU tests cover the writer; the GPU test runs
the benchmark and recomputes that step from the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _arrays(n):
    g = torch.Generator().manual_seed(3)
    return {"features": torch.randn(n, 64, 20, generator=g), "logits": torch.randn(n, 31, generator=g),
            "predictions": torch.randint(0, 31, (n,), generator=g)}


def _size(paths):
    return sum(os.path.getsize(p) for p in paths)


def test_dump_writes_float32_and_float64(tmp_path):
    arrs = _arrays(16)
    paths = bench.dump_outputs(str(tmp_path), arrs, bench.DUMP_LIMIT_BYTES)
    assert sorted(os.listdir(tmp_path)) == ["features.npy", "logits.npy", "predictions.npy"]
    assert _size(paths) <= bench.DUMP_LIMIT_BYTES
    for name, t in arrs.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == (np.float32 if t.dtype == torch.float32 else np.float64)
        assert np.array_equal(a, t.numpy().astype(a.dtype))


def test_dump_over_the_limit_keeps_one_seeded_sample_of_utterances(tmp_path):
    """Past the limit every array keeps the same utterances, chosen the same way on every run, and the files fit."""
    arrs = _arrays(64)
    limit = 20000
    first = bench.dump_outputs(str(tmp_path / "a"), arrs, limit, "_rank1")
    again = bench.dump_outputs(str(tmp_path / "b"), arrs, limit, "_rank1")
    assert _size(first) <= limit and _size(again) <= limit
    rows = np.load(tmp_path / "a" / "sample_rows_rank1.npy")
    assert rows.dtype == np.float64 and 1 <= len(rows) < 64 and (np.diff(rows) > 0).all()
    idx = rows.astype(np.int64)
    for name, t in arrs.items():
        a = np.load(tmp_path / "a" / f"{name}_rank1.npy")
        assert np.array_equal(a, t.numpy()[idx].astype(a.dtype))
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}_rank1.npy"))
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "c"), arrs, 500)


@pytest.mark.gpu
def test_dump_is_the_last_timed_step(tmp_path):
    """Timed step 2 * 3 - 1 = 5 of `--repeats 2 --steps 3` ran pool batch 5: the same clips, featurised and classified here
    outside the benchmark, give the dumped features and logits and identical predicted indices."""
    from sir_amd import synth
    from sir_amd.featurizer import get_featurizer
    from sir_amd.models.models import CNNAudioGRU
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--repeats", "2", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(bench.pick_json_line(r.stdout.splitlines()))
    # a plain run carries the timed regions only: every leg that takes runs of its own waits for --full
    assert d["timed_regions"]["repeats"] == 2 and d["ms_per_step"] > 0
    assert not {"roofline", "single_stream", "sustained", "train", "train_aug", "cpu_baseline", "parity"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["features.npy", "logits.npy", "predictions.npy"]
    feats, logits, pred = (np.load(tmp_path / f"{n}.npy") for n in ("features", "logits", "predictions"))

    dev = torch.device("cuda", 0)
    wave = bench.device_clips(bench.BATCH, bench.CLIP_LEN, 1234 + 5 % bench.N_POOL, dev)
    lengths = torch.full((bench.BATCH,), bench.CLIP_LEN, dtype=torch.int32, device=dev)
    model = CNNAudioGRU(bench.NUM_CLASSES)
    model.load_state_dict(synth.synth_state_dict(bench.NUM_CLASSES, seed=0))
    model = model.to(dev).eval()
    x = get_featurizer()(wave, lengths, t_pad=bench.T_PAD)
    ref_logits, ref_pred = model.predict(x)
    torch.cuda.synchronize()
    assert feats.shape == (bench.BATCH, 64, bench.T_PAD) and logits.shape == (bench.BATCH, bench.NUM_CLASSES)
    np.testing.assert_allclose(feats, x.cpu().numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(logits, ref_logits.cpu().numpy(), rtol=0, atol=1e-5)
    assert np.array_equal(pred, ref_pred.cpu().numpy().astype(np.float64))
