"""GPU: the plain `python bench.py --gpus 1 --steps K --warmup W` -- set-up, warm-up, K timed steps, the headline line and
nothing else -- and `--dump-outputs DIR`: the last timed step's logits and sampled token ids as .npy, identical inputs from run
to run.  A 2-layer stack of the smallest model at a small batch keeps it short; two runs of the same command side by side."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_elem_close

pytestmark = pytest.mark.gpu

B, STEPS, VOCAB = 5, 3, 151936


@pytest.mark.timeout(300)
def test_plain_run_prints_the_headline_and_dumps_what_the_last_step_computed(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
                               "--model", "qwen2-0.5b", "--quant", "none", "--layers", "2", "--batch", str(B), "--ctx", "70",
                               "--dump-outputs", d], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for d in dirs]
    outs = [p.communicate(timeout=280) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1, outs[0][0][-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["n_gpus"] == 1 and d["config"]["layers"] == 2
    assert d["unit"] == "tokens/s" and d["higher_is_better"] is True and d["dtype"] == "none" and "tokens/s" in d["metric"]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(B / d["ms_per_step"] * 1e3, rel=1e-3)
    # the side measurements belong to --full
    for key in ("roofline", "roofline_gemm", "ttft_ms_p50", "cpu_baseline", "other_configs", "value_fused", "median_step_ms_synced"):
        assert key not in d, key
    got = [{n: np.load(os.path.join(x, n + ".npy")) for n in ("logits", "next_token_ids")} for x in dirs]
    assert sorted(os.listdir(dirs[0])) == ["logits.npy", "next_token_ids.npy"]
    a, b = got
    assert a["logits"].dtype == np.float32 and a["logits"].shape == (B, VOCAB) and np.isfinite(a["logits"]).all()
    assert a["next_token_ids"].dtype == np.float64 and a["next_token_ids"].shape == (B,)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # the ids are the greedy sample of those logits (any of the tied maxima of a row): both arrays come from the same, last, step
    ids = a["next_token_ids"].astype(np.int64)
    assert np.array_equal(ids, a["next_token_ids"]) and np.array_equal(a["logits"][np.arange(B), ids], a["logits"].max(-1))
    # same arguments, same seeded inputs: the two runs agree (two 16-bit results of the same computation)
    assert np.array_equal(a["next_token_ids"], b["next_token_ids"])
    assert_elem_close(torch.from_numpy(a["logits"]), torch.from_numpy(b["logits"]), torch.bfloat16, pair=True,
                      what="logits of two runs of the same command")
