"""bench.py --dump-outputs / --full: the option defaults, and the writer of the
last timed step's output (the returned loss as a float32 .npy file)."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_dcp_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_options(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


_DIGEST = """
import hashlib, sys, torch
sys.path.insert(0, sys.argv[1])
from distributed_compute_pytorch_amd import workloads
torch.manual_seed(0)  # as bench.py seeds before it builds the workload
wl = workloads.build("resnet50", torch.device("cpu"), batch=2, fused=False)
h = hashlib.sha1()
for t in list(wl.model.parameters()) + list(wl.model.buffers()) + [t for b in wl.data.batches for t in b]:
    h.update(t.detach().contiguous().numpy().tobytes())
print(h.hexdigest())
"""


def test_bench_inputs_identical_from_run_to_run():
    """The flagship workload as bench.py builds it: weights, buffers and every
    synthetic batch are bit for bit the same in two fresh processes."""
    import subprocess

    env = dict(os.environ, DCP_NO_AUTOBUILD="1")
    runs = [subprocess.run([sys.executable, "-c", _DIGEST, REPO], capture_output=True, text=True, env=env, timeout=120)
            for _ in range(2)]
    assert all(r.returncode == 0 for r in runs), runs[0].stderr[-2000:] + runs[1].stderr[-2000:]
    a, b = (r.stdout.split()[-1] for r in runs)
    assert len(a) == 40 and a == b


def test_dump_outputs_writes_float32_loss(tmp_path):
    bench = _bench()
    out = tmp_path / "new" / "dir"
    bench._dump_outputs(str(out), torch.tensor(1.25, dtype=torch.bfloat16, requires_grad=True))
    assert os.listdir(out) == ["loss.npy"]
    got = np.load(out / "loss.npy")
    assert got.dtype == np.float32 and got.shape == (1,) and got.tolist() == [1.25]
    bench._dump_outputs(str(out), torch.tensor([2.5]))  # an existing directory: the file is replaced
    assert np.load(out / "loss.npy").tolist() == [2.5]
