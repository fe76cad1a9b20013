"""Graph D with deconv_final's channel sum folded into deconv0_b's epilogue (DenoiserEngine._fold_final; csrc/graph_exec.hip applies the
same rule): against the float64 oracle, image by image against the batch, the native executor against the Python engine bit for bit,
and the switch EMD_D_FOLD_FINAL=0 back on the pair of launches."""
import numpy as np
import pytest
import torch

from tests.synth_inputs import synthetic_lq
from tests.test_ops_gpu import dev, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def weights():
    import emdenoise

    return emdenoise.synthetic_weights()


def spy_engine(w, routes, **kw):
    import emdenoise

    class Spy(emdenoise.DenoiserEngine):
        def _fold_final(self, t):
            routes.append(super()._fold_final(t))
            return routes[-1]

    return Spy(w, dev(), "bf16x3", **kw)


@pytest.mark.parametrize("B,S", [(2, 64), (3, 64), (2, 96), (3, 96)])
def test_folded_engine_against_the_oracle_the_single_image_and_the_native_executor(B, S, weights, monkeypatch):
    from emdenoise.graph_exec import NativeGraph
    from oracle import denoiser_graph as GO

    monkeypatch.delenv("EMD_D_FOLD_FINAL", raising=False)
    routes = []
    eng = spy_engine(weights, routes)
    x_np = synthetic_lq(B, S, S, seed=300 + S)
    x = torch.from_numpy(x_np).to(dev())
    got = eng.forward(x).clone()
    torch.cuda.synchronize()
    assert routes and all(routes), "S % 16 == 0: the default route folds the final conv"
    ref = GO.architecture(x_np, weights, S, dtype=torch.float64).numpy()
    r = rel_l2(got.cpu().numpy(), ref)
    print(f"graph D [{B},{S},{S},1] folded vs the float64 oracle: rel_l2 = {r:.3e}")
    assert r < 3e-4
    for b in range(B):   # image b of a batch is the image alone
        alone = eng.forward(x[b:b + 1].contiguous()).clone()
        torch.cuda.synchronize()
        assert torch.equal(alone[0], got[b])
    nat = NativeGraph(weights, dev())
    try:
        native = nat.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(native, got)
    finally:
        nat.close()
    # the switch: today's pair of launches, bit for bit, and the two routes within rounding of each other
    monkeypatch.setenv("EMD_D_FOLD_FINAL", "0")
    off_routes = []
    off = spy_engine(weights, off_routes).forward(x).clone()

    import emdenoise

    class Pair(emdenoise.DenoiserEngine):
        def _fold_final(self, t):
            return False

    monkeypatch.delenv("EMD_D_FOLD_FINAL", raising=False)
    pair = Pair(weights, dev(), "bf16x3").forward(x).clone()
    torch.cuda.synchronize()
    assert off_routes and not any(off_routes)
    assert torch.equal(off, pair)
    d = rel_l2(got.cpu().numpy(), off.cpu().numpy())
    print(f"    folded vs the pair of launches: rel_l2 = {d:.3e}")
    assert d < 1e-5   # a sanity cap: in float64 the two are the same expression


def test_dprime_folded(monkeypatch):
    """The twin (act code 2: relu6 then the in-graph clip to [0, 1]) at S = 64: oracle, native executor, and the switch."""
    import emdenoise
    from emdenoise.graph_exec import NativeGraph

    monkeypatch.delenv("EMD_D_FOLD_FINAL", raising=False)
    w = emdenoise.synthetic_weights(variant="Dprime")
    routes = []
    eng = spy_engine(w, routes, variant="Dprime")
    x = torch.from_numpy(synthetic_lq(2, 64, 64, seed=364)).to(dev())
    got = eng.forward(x).clone()
    torch.cuda.synchronize()
    assert routes and all(routes)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    nat = NativeGraph(w, dev(), variant="Dprime")
    try:
        native = nat.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(native, got)
    finally:
        nat.close()
    monkeypatch.setenv("EMD_D_FOLD_FINAL", "0")
    off = emdenoise.DenoiserEngine(w, dev(), "bf16x3", variant="Dprime").forward(x).clone()
    torch.cuda.synchronize()
    d = rel_l2(got.cpu().numpy(), off.cpu().numpy())
    print(f"graph D' [2,64,64,1] folded vs the pair of launches: rel_l2 = {d:.3e}")
    assert d < 1e-5
