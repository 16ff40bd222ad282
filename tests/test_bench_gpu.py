"""GPU: bench.py --dump-outputs writes what the last timed step handed its caller, and two runs with the same arguments
write the same arrays (inputs, weights and dropout seeds are fixed by the arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, net, flags=("--no-cpu-baseline", "--no-extras")):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LTR_LIB")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--queries", "4096", "--batch", "1024",
                        "--steps", "3", "--warmup", "1", "--net", net, *flags, "--dump-outputs", out_dir],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("net", ["double", "triple"])
def test_bench_dump_outputs_are_the_last_step_and_reproducible(tmp_path, net):
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ja, jb = _bench(a, net), _bench(b, net)
    assert ja["steps"] == 3 and jb["steps"] == 3
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    params = dict((DoubleLayerNet(136) if net == "double" else TripleLayerNet(136)).named_parameters())
    want = ["loss.npy"] + [f"{kind}.{k}.npy" for k in params for kind in ("grad", "param")]
    assert names == sorted(want)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype, n
        assert np.array_equal(x, y), n
        total += x.nbytes
        if n != "loss.npy":
            k = n.split(".", 1)[1][:-len(".npy")]
            assert x.shape == tuple(params[k].shape), n
            assert np.isfinite(x).all(), n
    assert total <= 64 << 20
    loss = np.load(os.path.join(a, "loss.npy"))
    assert loss.shape == (1,) and round(float(loss[0]), 6) == ja["config"]["final_loss"]
    assert np.abs(np.load(os.path.join(a, f"grad.{next(iter(params))}.npy"))).max() > 0


@pytest.mark.timeout(900)
def test_bench_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    """A plain run prints the headline line without the CPU baseline or the secondary lines; --full adds the CPU baseline
    (--no-extras keeps the secondary child runs out of this test) and leaves the dumped arrays of the same steps unchanged."""
    a, b = str(tmp_path / "plain"), str(tmp_path / "full")
    plain, full = _bench(a, "double", flags=()), _bench(b, "double", flags=("--full", "--no-extras"))
    assert "cpu_baseline" not in plain and "secondary" not in plain
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["unit"] == "slates/s" and "secondary" not in full
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["config"]["final_loss"] == full["config"]["final_loss"]
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    for n in names:
        assert np.array_equal(np.load(os.path.join(a, n)), np.load(os.path.join(b, n))), n
