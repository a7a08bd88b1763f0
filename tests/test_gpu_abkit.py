"""tools/abkit.py on the device: capture_step / replay_ms / interleave (through ab_step) driven by one small conv.  Each captured graph is one
stream, no parallel branches inside.  Nothing is asserted about speed."""
import importlib.util
import math
import os

import pytest
import torch

from step_amd import _capi, _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("abkit", os.path.join(ROOT, "tools", "abkit.py"))
abkit = importlib.util.module_from_spec(spec)
spec.loader.exec_module(abkit)


def test_ab_step_on_one_small_conv():
    dev = torch.device("cuda:0")
    product = _lib.lib()
    product.step_reset_options()
    defaults = {k: _capi.get_option(product, k) for k in _capi.OPTION_IDS}
    g = torch.Generator(device="cpu").manual_seed(3)
    xs = [torch.randn(1, 2, 8, 8, 16, generator=g).to(dev).to(torch.bfloat16) for _ in range(2)]
    w = ops.pack_conv_weight((torch.randn(16, 16, 3, 3, 3, generator=g) / (16 * 27) ** 0.5).to(dev), torch.bfloat16)
    sc, sh = torch.ones(16, device=dev), torch.zeros(16, device=dev)
    fn = lambda x: ops.conv_forward(x, w, 16, (3, 3, 3), sc, sh, True)
    variants = [abkit.Variant.parse(t) for t in ("default", "default", "conv_waves=4")]
    same, times = abkit.ab_step(fn, xs, variants, in_flight=(1, 2), rounds=2, steps=3)
    assert len(same) == len(times) == 3
    assert same[0] == (True, 0.0) and same[1] == (True, 0.0)                 # default against default: the same bits
    assert math.isfinite(same[2][1])
    for t in times:
        assert set(t) == {1, 2}
        for leg in t.values():
            assert len(leg) == 2 and list(leg) == sorted(leg) and leg.median == leg[1] and leg.min == leg[0]
            assert all(math.isfinite(v) and v > 0 for v in leg)
    assert {k: _capi.get_option(product, k) for k in _capi.OPTION_IDS} == defaults
    assert _lib.lib() is product
