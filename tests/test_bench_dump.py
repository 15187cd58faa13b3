"""bench.py --dump-outputs on the host: what dump_outputs writes (names, dtypes, the seeded sample, the size budget) and the argument
checks that run before bench.py looks for a GPU.  The GPU run of the flag is in tests/test_bench_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import torch
from transformers.modeling_outputs import BaseModelOutputWithPooling

import bench
from cm3p_amd.modeling_cm3p import CM3POutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step_output():
    g = torch.Generator().manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.Linear(4, 2, bias=False))
    model[1].weight.requires_grad_(False)  # a parameter without a gradient is left out
    model(torch.randn(3, 8, generator=g)).sum().backward()
    big = torch.randn(3, bench.DUMP_SAMPLE + 5, generator=g)
    out = CM3POutput(loss=torch.tensor(1.25), logits_per_beatmap=torch.randn(3, 3, generator=g).bfloat16(),
                     metadata_embeds=torch.randn(3, 4, generator=g, dtype=torch.float64),
                     beatmap_model_output=BaseModelOutputWithPooling(last_hidden_state=big, pooler_output=torch.arange(6).view(3, 2)))
    return out, model, big


def test_dump_outputs_writes_every_output_and_the_gradients(tmp_path):
    out, model, big = _step_output()
    written = bench.dump_outputs(str(tmp_path), out, model)
    names = {"loss", "logits_per_beatmap", "metadata_embeds", "beatmap_model_output.last_hidden_state", "beatmap_model_output.pooler_output",
             "grad_sample", "grad_norm"}
    assert set(written) == names and {f[:-4] for f in os.listdir(tmp_path)} == names
    a = {n: np.load(tmp_path / f"{n}.npy") for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["loss"].shape == () and a["loss"] == np.float32(1.25)
    assert a["logits_per_beatmap"].dtype == np.float32 and a["logits_per_beatmap"].shape == (3, 3)
    np.testing.assert_array_equal(a["logits_per_beatmap"], out.logits_per_beatmap.float().numpy())
    assert a["metadata_embeds"].dtype == np.float64
    np.testing.assert_array_equal(a["beatmap_model_output.pooler_output"], np.arange(6, dtype=np.float64).reshape(3, 2))  # integers: float64
    grads = [model[0].weight.grad, model[0].bias.grad]  # named_parameters() order, the frozen weight skipped
    np.testing.assert_array_equal(a["grad_sample"], torch.cat([g.reshape(-1) for g in grads]).numpy())  # small enough: all of it
    np.testing.assert_allclose(a["grad_norm"], [g.double().norm().item() for g in grads], rtol=1e-12)
    # the large tensor: DUMP_SAMPLE of its elements, the same ones on every call
    s = a["beatmap_model_output.last_hidden_state"]
    assert s.shape == (bench.DUMP_SAMPLE,) and s.dtype == np.float32
    assert np.isin(s[:1000], big.numpy()).all()
    bench.dump_outputs(str(tmp_path / "again"), out, model)
    np.testing.assert_array_equal(np.load(tmp_path / "again" / "beatmap_model_output.last_hidden_state.npy"), s)


def test_dump_sample_fits_the_budget_for_the_largest_workload():
    """Every output tensor and the gradient sample at their caps stay inside 64 MB with room for the step's outputs (at most a dozen
    tensors in any workload of bench.py)."""
    assert bench.DUMP_GRAD_SAMPLE * 4 + 12 * bench.DUMP_SAMPLE * 4 <= bench.DUMP_BUDGET_BYTES


def test_bench_refuses_a_step_count_below_one():
    for args in (["--steps", "0"], ["--warmup", "-1"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-2000:]
