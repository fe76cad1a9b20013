"""Graph S training on the GPU (emdenoise.AutoencoderTrainer) against the float64 restatement (tests/s_train_ref.py): gradients,
the Adam trajectory, the device sampler, the fused head, captured against eager steps, checkpoints through
Micrograph_Autoencoder, resume, and a short learning check."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RESUME_BAR = 5e-3   # captured against eager, and resume against uninterrupted (steps are not bitwise reproducible)


def _dev():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mods():
    import emdenoise
    from emdenoise import autoencoder_trainer as AT
    from tests import s_train_ref as R

    return emdenoise, AT, R


def _batch(B, S, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S] / S
    base = 1.0 + 0.5 * np.sin(6 * yy[None] + 4 * xx[None] + rng.random((B, 1, 1)) * 6)
    return (base + 0.3 * rng.standard_normal((B, S, S))).astype(np.float32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-300))


# encoding_features 1 at [2,32,32] is held by tests/test_s_train_teacher_gpu.py instead: free running, the first block's
# pointwise gradient (one input channel: a scale a batch norm removes, so its gradient exists only through eps and is tiny)
# measured 0.49 rel L2 at cosine 0.99993 with 4 flipped relu units; on the oracle's forward values 2.1e-5
@pytest.mark.parametrize("enc,B,S", [(4, 2, 32), (16, 2, 32), (1, 4, 160), (4, 4, 160), (16, 4, 160)])
def test_gradients_vs_float64(enc, B, S):
    dev = _dev()
    emdenoise, AT, R = _mods()
    w = emdenoise.autoencoder.synthetic_weights(enc, 21)
    x = _batch(B, S, 3 + enc)
    tr = AT.AutoencoderTrainer(enc, device=dev, initial=w)
    loss, g = tr.loss_and_grad(x)
    rloss, rg = R.loss_and_grads(x, w, enc)
    assert abs(loss - rloss) / rloss <= 1e-5, (loss, rloss)
    zero = set(AT.zero_gradient_names(enc))
    # Free running: worst tensor 2.2e-2 rel L2 / cosine 0.99981 at [2,32,32], 7e-3 at [4,160,160]; the loss agrees to 1e-5.  The
    # cause is the forward's split-bf16 values acting through the relu masks (1-4 flipped units at [2,32,32], 61-78 at
    # [4,160,160]) and the batch norms: on the oracle's forward values the same reverse pass agrees to 3.4e-5 with no flips, and
    # every layer on its own to 1e-5 (tests/test_s_train_teacher_gpu.py).
    # Gradients that exist only through eps (a weight feeding a batch norm is scale-invariant but for eps: the first block's
    # pointwise weights with ONE input channel, the normalizer gammas) are tiny and lose their relative precision to cancellation
    # in float32; below 1e-3 of the largest gradient they are held to an absolute bar against that largest gradient.
    top = max(np.linalg.norm(v) for v in rg.values())
    bad = []
    for n, ref in rg.items():
        assert g[n].shape == ref.shape, n
        if n in zero:
            assert np.all(g[n] == 0), n
            continue
        if np.linalg.norm(ref) < 1e-3 * top:
            if np.linalg.norm(g[n] - ref) > 1e-5 * top:
                bad.append((n, "abs", np.linalg.norm(g[n] - ref) / top))
            continue
        r, c = _rel(g[n], ref), _cos(g[n], ref)
        if r > 3e-2 or c < 0.9995:
            bad.append((n, r, c))
    assert not bad, bad


@pytest.mark.parametrize("Cc,H,W", [(4, 37, 45), (8, 9, 33), (16, 17, 70), (32, 8, 31), (128, 21, 40), (256, 13, 19)])
def test_fused_head_channels_and_tails(Cc, H, W):
    """Every channel-quad instantiation and image sizes that are not multiples of the 8 x 32 tile, against float64."""
    import torch

    dev = _dev()
    emdenoise, AT, R = _mods()
    from emdenoise import ops

    rng = np.random.default_rng(Cc + H)
    B = 2
    a = torch.from_numpy(np.maximum(rng.standard_normal((B, H, W, Cc)), 0).astype(np.float32)).to(dev)
    out = torch.from_numpy(rng.standard_normal((B, H, W)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((B, H, W)).astype(np.float32)).to(dev)
    w9 = torch.from_numpy((rng.standard_normal((9, Cc)) * 0.1).astype(np.float32)).to(dev)
    dw, db, loss = torch.zeros(9, Cc, device=dev), torch.zeros(Cc, device=dev), torch.zeros(1, device=dev)
    da = AT.head_backward(out, x, ops.Act(a.clone()), w9, dw, db, loss, fused=True).torch().cpu().numpy()
    a64, e = a.cpu().double(), (out - x).cpu().double()
    n = e.numel()
    dout = torch.nn.functional.pad(2 * e / n, (1, 1, 1, 1))
    w64 = w9.cpu().double()
    g = sum(dout[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, None] * w64[3 * ky + kx] for ky in range(3) for kx in range(3))
    da_ref = torch.where(a64 > 0, g, torch.zeros_like(g))
    ap = torch.nn.functional.pad(a64, (0, 0, 1, 1, 1, 1))
    dw_ref = torch.stack([(ap[:, ky:ky + H, kx:kx + W] * (2 * e / n)[..., None]).sum((0, 1, 2)) for ky in range(3) for kx in range(3)])
    assert _rel(da, da_ref) <= 1e-6 and _rel(dw.cpu().numpy(), dw_ref) <= 1e-6
    assert _rel(db.cpu().numpy(), da_ref.sum((0, 1, 2))) <= 1e-5
    assert abs(float(loss[0]) - float((e ** 2).mean())) <= 1e-6 * float((e ** 2).mean())


def test_fused_head_matches_composed():
    import torch

    dev = _dev()
    emdenoise, AT, R = _mods()
    from emdenoise import ops

    rng = np.random.default_rng(5)
    B, S, Cc = 3, 48, 64
    a = torch.from_numpy(np.maximum(rng.standard_normal((B, S, S, Cc)), 0).astype(np.float32)).to(dev)
    out = torch.from_numpy(rng.standard_normal((B, S, S)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((B, S, S)).astype(np.float32)).to(dev)
    w9 = torch.from_numpy((rng.standard_normal((9, Cc)) * 0.1).astype(np.float32)).to(dev)
    res = []
    for fused in (True, False):
        dw, db, loss = torch.zeros(9, Cc, device=dev), torch.zeros(Cc, device=dev), torch.zeros(1, device=dev)
        da = AT.head_backward(out, x, ops.Act(a.clone()), w9, dw, db, loss, fused=fused)
        res.append([t.cpu().numpy() for t in (da.torch(), dw, db, loss)])
    for f, c in zip(*res):
        assert _rel(f, c) <= 1e-6
    # the float64 statement of the same pass
    a64, e = a.cpu().double(), (out - x).cpu().double()
    n = e.numel()
    dout = torch.nn.functional.pad(2 * e / n, (1, 1, 1, 1))
    w64 = w9.cpu().double()
    g = sum(dout[:, 2 - ky:2 - ky + S, 2 - kx:2 - kx + S, None] * w64[3 * ky + kx] for ky in range(3) for kx in range(3))
    da_ref = torch.where(a64 > 0, g, torch.zeros_like(g))
    ap = torch.nn.functional.pad(a64, (0, 0, 1, 1, 1, 1))
    dw_ref = torch.stack([(ap[:, ky:ky + S, kx:kx + S] * (2 * e / n)[..., None]).sum((0, 1, 2)) for ky in range(3) for kx in range(3)])
    assert _rel(res[0][0], da_ref) <= 1e-6 and _rel(res[0][1], dw_ref) <= 1e-6
    assert _rel(res[0][2], da_ref.sum((0, 1, 2))) <= 1e-5
    assert abs(float(res[0][3][0]) - float((e ** 2).mean())) <= 1e-6 * float((e ** 2).mean())


def test_adam_trajectory():
    dev = _dev()
    emdenoise, AT, R = _mods()
    enc = 4
    w = emdenoise.autoencoder.synthetic_weights(enc, 8)
    batches = [_batch(2, 32, 100 + k) for k in range(4)]
    tr = AT.AutoencoderTrainer(enc, device=dev, initial=w)
    for t in range(20):
        tr.train_step(batches[t % 4])
    got = tr.weights()
    zero = AT.zero_gradient_names(enc)
    ref = R.adam_trajectory(batches, w, enc, lambda t: AT.lr_schedule(t), 20, zero=zero)
    for n in zero:
        np.testing.assert_array_equal(got[n], w[n])
    # measured worst 7.9e-3 (the gradient error above, carried through 20 steps); DESIGN.md 3.12
    bad = [(n, _rel(got[n], ref[n])) for n in ref if _rel(got[n], ref[n]) > 2e-2]
    assert not bad, bad
    for n, v in got.items():
        if n.endswith(("/moving_mean", "/moving_variance")):
            np.testing.assert_array_equal(v, w[n])


def test_sampler_matches_host():
    import torch

    dev = _dev()
    emdenoise, AT, R = _mods()
    from emdenoise import k_trainer as KT

    rng = np.random.default_rng(4)
    stack = rng.random((5, 171, 180)).astype(np.float32) * 3
    stack[2] = np.nan                       # an all-NaN image: constant -> 0.5 -> ones
    stack[3, ::2] = 3e38                    # overflowing range: non-finite after scale0to1 -> ones (graph S)
    stack[3, 1::2] = -3e38
    sd = torch.from_numpy(stack).to(dev)
    B = 24
    draws = torch.empty((B, 4), dtype=torch.int32, device=dev)
    x4 = torch.zeros((B, 160, 160, 4), dtype=torch.float32, device=dev)
    out = AT.sample_crops(sd, B, 160, 7, 96, x4=x4, draws=draws)
    out, x4, dr = out.cpu().numpy(), x4.cpu().numpy(), draws.cpu().numpy()
    np.testing.assert_array_equal(x4[..., 0], out)
    assert np.all(x4[..., 1:] == 0)
    seen = set()
    for b in range(B):
        n, x, y, ch = (int(v) for v in dr[b])
        assert 0 <= n < 5 and 0 <= x < 11 and 0 <= y < 20 and 0 <= ch < 8
        seen.add(n)
        ref = AT.s_crop(stack[n], x, y, ch, 160)
        if n in (2, 3):
            np.testing.assert_array_equal(out[b], np.ones((160, 160), np.float32))
        assert _rel(out[b], ref) <= 1e-6, b
    assert 3 in seen        # the non-finite fallback itself (image 2 reaches ones through the constant-crop path)
    one = AT.sample_crops(torch.from_numpy(np.ascontiguousarray(stack[3:4])).to(dev), 4, 160, 1, 0).cpu().numpy()
    np.testing.assert_array_equal(one, np.ones((4, 160, 160), np.float32))
    # the K sampler keeps its zeros fallback and its own stream
    kd = torch.empty((B, 4), dtype=torch.int32, device=dev)
    kc = KT.sample_crops(sd, B, 160, 7, 96, draws=kd).cpu().numpy()
    kd = kd.cpu().numpy()
    for b in range(B):
        n, x, y, ch = (int(v) for v in kd[b])
        assert _rel(kc[b], KT.k_crop(stack[n], x, y, ch, 160)) <= 1e-6 or (n == 3 and np.all(kc[b] == 0))
    assert not np.array_equal(kd, dr)


def _train_pair(enc, steps, graph_a, graph_b, dev, AT, stack):
    res = []
    for graph in (graph_a, graph_b):
        tr = AT.AutoencoderTrainer(enc, device=dev, seed=3)
        tr.train(stack, steps, batch_size=4, graph=graph)
        res.append(tr)
    return res


def test_captured_matches_eager():
    dev = _dev()
    emdenoise, AT, R = _mods()
    stack = _batch(6, 171, 12)
    a, b = _train_pair(16, 5, False, True, dev, AT, stack)
    wa, wb = a.weights(), b.weights()
    worst = max(_rel(wb[n], wa[n]) for n in wa if np.any(wa[n]))
    print(f"captured vs eager after 5 steps: worst rel L2 {worst:.3e}, bitwise {all(np.array_equal(wa[n], wb[n]) for n in wa)}")
    # not bitwise: the depthwise and final-conv weight gradients add with float atomics, and Adam normalises that rounding
    # noise where a gradient is small; measured worst tensor 1.0e-3 after 5 steps
    assert worst <= RESUME_BAR


def test_checkpoint_apply_and_resume(tmp_path):
    import torch

    dev = _dev()
    emdenoise, AT, R = _mods()
    from emdenoise import autoencoder

    enc = 4
    stack = _batch(8, 171, 31)
    tr = AT.AutoencoderTrainer(enc, device=dev, seed=5)
    tr.train(stack, 3, batch_size=4)
    d = str(tmp_path / "ckpt")
    tr.save_checkpoint(d)
    m = autoencoder.Micrograph_Autoencoder(checkpoint_loc=d, encoding_features=enc)
    crop = stack[0, :160, :160]
    ref = autoencoder.Micrograph_Autoencoder(weights=tr.weights(), encoding_features=enc)
    np.testing.assert_array_equal(m.denoise_crop(crop), ref.denoise_crop(crop))
    xin = torch.from_numpy(_batch(2, 160, 2)[..., None]).to(dev)
    np.testing.assert_array_equal(m.engine.forward(xin).cpu().numpy(), tr.engine().forward(xin).cpu().numpy())
    # resume: 3 + 2 steps against 5 uninterrupted
    tr.train(stack, 2, batch_size=4)
    r = AT.AutoencoderTrainer(enc, device=dev, seed=5)
    assert r.restore(d).endswith("-3") and r.step == 3
    r.train(stack, 2, batch_size=4)
    wa, wb = tr.weights(), r.weights()
    worst = max(_rel(wb[n], wa[n]) for n in wa if np.any(wa[n]))
    assert worst <= RESUME_BAR, worst
    # padded channels (encoding_features < 4, the one-channel input) are not parameters and stay zero
    t1 = AT.AutoencoderTrainer(1, device=dev, seed=1)
    t1.train(stack, 2, batch_size=2)
    flat = t1.params.cpu().numpy()
    for name in t1.trainable:
        off, canon, padded = t1._offs[name]
        buf = flat[off: off + int(np.prod(padded))].reshape(padded).copy()
        buf[tuple(slice(0, c) for c in canon)] = 0
        assert np.all(buf == 0), name
    sd = t1.state_dict()
    assert set(sd) == set(AT.state_dict_names(1)) and sd["Conv2d_transpose/weights"].shape == (3, 3, 256, 1)


def test_guards():
    dev = _dev()
    emdenoise, AT, R = _mods()
    tr = AT.AutoencoderTrainer(4, device=dev, total_steps=2, period=1)
    x = _batch(2, 32, 1)
    tr.train_step(x)
    tr.train_step(x)
    with pytest.raises(ValueError):
        tr.train_step(x)
    with pytest.raises(ValueError):
        tr.loss_and_grad(_batch(2, 30, 1))


def test_short_learning_check():
    dev = _dev()
    emdenoise, AT, R = _mods()
    tr = AT.AutoencoderTrainer(16, device=dev, seed=0)
    out = tr.train(_batch(8, 171, 77), 200, batch_size=8)
    loss = out["loss"]
    print(f"200 steps at [8,160,160]: loss {loss[0]:.4f} -> {loss[-10:].mean():.4f}")
    assert np.all(np.isfinite(loss)) and loss[-10:].mean() < loss[0]
