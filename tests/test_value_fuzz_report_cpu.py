"""The fuzz legs' value-first check (tools/lab/value_fuzz.py judge_launch / value_first), without a GPU: each of two launches is held to the
fp64 reference at the leg's bound before the two are compared, and a failure names the launch that is off (first, second, both), the worst
(batch, head, row), that row's error and the LSE error -- planted errors here must be found where they were put."""
import importlib.util
import re
from pathlib import Path

import pytest

torch = pytest.importorskip("torch")
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def vf():
    spec = importlib.util.spec_from_file_location("value_fuzz", ROOT / "tools" / "lab" / "value_fuzz.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(B=2, H=3, Sq=5, Skv=40, D=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, H, n, D, generator=g, dtype=torch.float64) for n in (Sq, Skv, Skv))
    s = q @ k.transpose(-1, -2) * D ** -0.5
    ref, rl = torch.softmax(s, dim=-1) @ v, torch.logsumexp(s, dim=-1)
    return ref, rl


def _worst(msg):
    return tuple(int(x) for x in re.search(r"\(b (\d+), h (\d+), row (\d+)\)", msg).groups())


def test_exact_launches_pass(vf):
    ref, rl = _case()
    o = ref.float()
    assert vf.value_first([(o, rl.float()), (o.clone(), None)], ref, rl, 1e-3, 1e-3, "what") is None
    assert vf.value_first([(o, rl.float()), (o.clone(), None)], ref, rl, 1e-3, 1e-3, "what", per_slab=True) is None


def test_second_launch_off_at_a_planted_row(vf):
    ref, rl = _case()
    o1 = ref.float()
    o2 = o1.clone()
    o2[1, 2, 3, 7] += 0.01 * float(ref.abs().max())
    msg = vf.value_first([(o1, rl.float()), (o2, None)], ref, rl, 1e-3, 1e-3, ("seed", "kern<x>"))
    assert msg.startswith("the second launch off"), msg
    assert "first:" not in msg and _worst(msg) == (1, 2, 3) and "kern<x>" in msg
    assert re.search(r"rel 1\.0\d\de-02", msg), msg


def test_both_launches_off_and_non_finite(vf):
    ref, rl = _case()
    o1, o2 = ref.float(), ref.float()
    o1[0, 1, 4, 0] = float("nan")
    o2[1, 0, 0, 3] *= 1.5
    msg = vf.value_first([(o1, rl.float()), (o2, None)], ref, rl, 1e-3, 1e-3, "w")
    assert msg.startswith("both launches off"), msg
    first, second = msg.split("; second: ")
    assert "non-finite rows 1" in first and _worst(first) == (0, 1, 4)
    assert _worst(second) == (1, 0, 0)


def test_lse_and_dead_rows(vf):
    ref, rl = _case()
    o = ref.float()
    bad_lse = rl.float().clone()
    bad_lse[0, 0, 2] += 0.5
    msg = vf.value_first([(o, bad_lse), (o.clone(), None)], ref, rl, 1e-3, 1e-3, "w")
    assert msg.startswith("the first launch off") and "lse 1.0" in msg, msg  # (|0.5| / max(|lse|, 50))
    assert vf.value_first([(o, bad_lse), (o.clone(), None)], ref, rl, 1e-3, None, "w") is None  # lbound None: reported, not judged
    # a row without a key: O must be 0 and (judged LSE) -inf
    ref2, rl2 = ref.clone(), rl.clone()
    ref2[1, 1, 1] = 0.0
    rl2[1, 1, 1] = float("-inf")
    o2 = ref2.float()
    l2 = rl2.float()
    assert vf.value_first([(o2, l2), (o2.clone(), None)], ref2, rl2, 1e-3, 1e-3, "w", dead=True) is None
    l3 = l2.clone()
    l3[1, 1, 1] = 0.0
    assert "dead rows NOT" in vf.value_first([(o2, l3), (o2.clone(), None)], ref2, rl2, 1e-3, 1e-3, "w", dead=True)


def test_per_slab_scale(vf):
    """per (batch, head) slab: an error that is small against the whole tensor's largest value but large against its own slab is found"""
    ref, rl = _case()
    ref = ref.clone()
    ref[0, 2] *= 1e-3
    o = ref.float()
    o[0, 2, 1, 5] += 1e-2 * float(ref[0, 2].abs().max())
    assert vf.value_first([(o, None), (o.clone(), None)], ref, rl, 1e-3, None, "w") is None
    msg = vf.value_first([(o, None), (o.clone(), None)], ref, rl, 1e-3, None, "w", per_slab=True)
    assert msg.startswith("both launches off") and _worst(msg) == (0, 2, 1), msg
