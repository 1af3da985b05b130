"""bench.py's run options: a plain run prints only the headline line, `--full` adds the figures that take runs of their own,
`--dump-outputs DIR` writes what the last timed step computed (float32 / float64 .npy, large arrays as a fixed seeded sample)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_types_sampling_and_budget(tmp_path):
    import bench
    big = np.arange(bench.DUMP_WHOLE_ELEMS + 7, dtype=np.float32).reshape(-1, 1)
    outs = {"loss": np.float64(0.25), "params": np.ones(10, np.float32), "labels": np.zeros((2, 3), np.int32), "big": big}
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in outs}
    assert a["loss"].dtype == np.float64 and a["loss"] == 0.25
    assert a["params"].dtype == np.float32 and a["params"].shape == (10,)
    assert a["labels"].dtype == np.float32 and a["labels"].shape == (2, 3)
    assert a["big"].shape == (bench.DUMP_SAMPLE_ELEMS,) and np.all(np.diff(a["big"]) >= 0)
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))          # the same positions every run
    with pytest.raises(RuntimeError, match="budget"):
        bench.dump_outputs({f"w{i}": np.zeros(bench.DUMP_WHOLE_ELEMS, np.float32) for i in range(5)}, str(tmp_path / "c"))


def test_steps_below_one_is_an_argument_error():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 2 and "--steps" in r.stderr.decode()


@pytest.mark.gpu
def test_plain_run_headline_only_and_dump_of_the_last_step(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--dump-outputs", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-4000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["unit"] == "images/sec" and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert out["value"] > 0 and np.isclose(out["value"], 4 * 1e3 / out["ms_per_step"], rtol=1e-2)
    assert not {"roofline", "kernels_survey_step", "nms_boxes_per_sec", "cpu_baseline"} & set(out)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert {"loss", "output-mask_loss", "output-labels_loss", "output-boxes_loss", "output-labels", "output-boxes", "params", "grads",
            "state"} <= set(got)
    assert got["params"].shape == (4009920,) and got["output-labels"].shape == (4, 9600, 4)
    assert all(np.isfinite(a).all() for a in got.values())
    assert np.abs(got["output-labels"].sum(-1) - 1).max() < 1e-4
