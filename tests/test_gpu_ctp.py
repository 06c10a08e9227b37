"""The CTP-conditioned CAE on the GPU: the stack-input kernel (csrc/sp_ctp.hip) against the torch composition it replaces,
``Enc3DCtp`` against ``Enc3D(channels[0] = 3)`` fed the concatenated inputs, the f32 mode against the fixture recorded from the
reference's ``Cae3DCtp`` (tests/golden/make_golden_ctp.py), training through ``CaeReconstructionLearner`` (eager, captured,
pass by pass) and the training script."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import weights as W
import stroke_prediction_amd  # noqa: F401
import common.dto.CaeDto as CaeDtoUtil
from stroke_prediction_amd.common.model.Cae3D import Cae3DCtp, Dec3D, Enc3D, Enc3DCtp
from stroke_prediction_amd.common.metrics import BatchDiceLoss
from stroke_prediction_amd.learner.CaeReconstructionLearner import CaeReconstructionLearner
from stroke_prediction_amd.optim import FusedAdam
from stroke_prediction_amd.runtime import lib as L, ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CH = [3, 16, 24, 32, 100, 200, 1]


def ctp_inputs(seed, d, hw, padding):
    """the padded CBV / TTD volumes of tests/golden/make_golden_ctp.py (same recipe)"""
    seg, _ = W.cae_inputs(2, d, hw, seed + 11)
    cbv = 0.05 + 0.6 * seg[:, 0:1] + 0.3 * seg[:, 2:3]
    ttd = 0.05 + 0.9 * seg[:, 1:2]
    pd, ph, pw = padding
    pad = lambda t: F.pad(t, (pw, pw, ph, ph, pd, pd)).contiguous()
    return pad(cbv), pad(ttd)


def _crop(t, offs, dims):
    (od, oh, ow), (D, H, W_) = offs, dims
    return t[:, :, od:od + D, oh:oh + H, ow:ow + W_]


# ------------------------------------------------------------------------------------------------ the kernel
def _torch_stack_input(labels, cbv, ttd, offs, cp, tdt):
    """crop -> cat -> permute -> channel pad -> cast: what StackContext built before, as one torch expression"""
    dims = tuple(labels[0].shape[2:])
    c, t = _crop(cbv, offs, dims), _crop(ttd, offs, dims)
    x = torch.cat([torch.cat([lab, c, t], 1) for lab in labels], 0).permute(0, 2, 3, 4, 1)
    return F.pad(x, (0, cp - 3)).to(tdt).contiguous()


@pytest.mark.parametrize("dtype", [L.SP_BF16, L.SP_F32])
@pytest.mark.parametrize("G,B,dims,pad", [(3, 3, (7, 9, 13), (1, 2, 0)), (1, 3, (7, 9, 13), (0, 3, 1)),
                                          (3, 4, (28, 128, 128), (20, 20, 20))])
def test_stack_input_kernel_matches_the_torch_composition(dtype, G, B, dims, pad):
    g = torch.Generator(device="cpu").manual_seed(5)
    D, H, W_ = dims
    labs = (torch.rand((B, 3) + dims, generator=g) > 0.6).float().to(DEV)
    labels = [labs[:, k:k + 1] for k in range(3)][:G] if G == 3 else [labs[:, 1:2]]        # views: batch stride 3 DHW
    assert labels[0].stride(0) == 3 * D * H * W_
    pdims = (D + 2 * pad[0], H + 2 * pad[1], W_ + 2 * pad[2])
    imgs = (0.05 + 0.9 * torch.rand((B, 2) + pdims, generator=g)).to(DEV)
    cbv, ttd = imgs[:, 0:1], imgs[:, 1:2]
    cp = 16 if dtype == L.SP_BF16 else 8
    tdt = O.TORCH_DT[dtype]
    nrep = 64
    x0 = torch.full((G * B,) + dims + (cp,), 7.0, dtype=tdt, device=DEV)
    sums = torch.zeros(G * nrep * cp * 2, dtype=torch.float64, device=DEV)
    O.ctp_stack_input(labels, cbv, ttd, pad, x0, dtype, sums, nrep * cp * 2, nrep)
    ref = _torch_stack_input(labels, cbv, ttd, pad, cp, tdt)
    bits = torch.int16 if dtype == L.SP_BF16 else torch.int32
    assert torch.equal(x0.view(bits), ref.view(bits))
    assert not x0[..., 3:].float().abs().any()
    st = sums.view(G, nrep, cp, 2).sum(1)
    stored = ref[..., :3].double().reshape(G, -1, 3)
    want = torch.stack([stored.sum(1), (stored * stored).sum(1)], -1)
    torch.testing.assert_close(st[:, :3], want, rtol=1e-12, atol=1e-9)
    assert not st[:, 3:].any()
    # eval: no statistics
    x1 = torch.empty_like(x0)
    O.ctp_stack_input(labels, cbv, ttd, pad, x1, dtype)
    assert torch.equal(x1.view(bits), ref.view(bits))


def test_eval_forward_leaves_the_first_accumulator_untouched():
    d, hw, pad = 28, 64, (2, 0, 4)
    enc = Enc3DCtp(hw, d, CH, 5, 1.0, pad, dtype="bf16").to(DEV).eval()
    labels, _ = W.cae_inputs(2, d, hw, 3)
    cbv, ttd = ctp_inputs(3, d, hw, pad)
    labels, cbv, ttd = labels.to(DEV), cbv.to(DEV), ttd.to(DEV)
    dto = CaeDtoUtil.init_dto(None, torch.full((2, 1, 1, 1, 1), 0.3, device=DEV), None, None, cbv, ttd,
                              labels[:, 0:1], labels[:, 1:2], labels[:, 2:3])
    with torch.no_grad():
        enc(dto)
    ctxs = [sc for lst in enc._stack_pool.free.values() for sc in lst]
    assert len(ctxs) == 1 and ctxs[0].G == 3
    sc = ctxs[0]
    assert not sc.layers[0].in_sums.any()
    ref = _torch_stack_input([labels[:, k:k + 1] for k in range(3)], cbv, ttd, pad, 16, torch.bfloat16)
    assert torch.equal(sc.x0.view(torch.int16), ref.view(torch.int16))
    assert dto.latents.inputs._is_empty()


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("batched", [1, 0])
def test_latents_and_gradients_equal_enc3d_on_concatenated_inputs(batched, monkeypatch):
    import stroke_prediction_amd.common.model.Cae3D as M
    monkeypatch.setattr(M, "CAE_BATCHED", batched)
    d, hw, pad, seed = 28, 64, (2, 0, 4), 13
    sd = W.make_state_dict(W.enc_spec(CH), seed)
    ctp = Enc3DCtp(hw, d, CH, 5, 1.0, pad, dtype="f32")
    ref = Enc3D(hw, d, CH, 5, 1.0, dtype="f32")
    ctp.load_state_dict(sd)
    ref.load_state_dict(sd)
    ctp, ref = ctp.to(DEV).train(), ref.to(DEV).train()
    labels, _ = W.cae_inputs(2, d, hw, seed)
    cbv, ttd = ctp_inputs(seed, d, hw, pad)
    labels, cbv, ttd = labels.to(DEV), cbv.to(DEV), ttd.to(DEV)
    step = torch.full((2, 1, 1, 1, 1), 0.4, device=DEV)
    gts = [labels[:, k:k + 1] for k in range(3)]
    c, t = _crop(cbv, pad, (d, hw, hw)), _crop(ttd, pad, (d, hw, hw))
    a = ctp(CaeDtoUtil.init_dto(None, step, None, None, cbv, ttd, *gts))
    b = ref(CaeDtoUtil.init_dto(None, step, None, None, None, None, *[torch.cat([x, c, t], 1) for x in gts]))
    g = torch.Generator(device="cpu").manual_seed(1)
    loss_a = loss_b = 0.0
    for k in ("core", "penu", "lesion", "interpolation"):
        la, lb = getattr(a.latents.gtruth, k), getattr(b.latents.gtruth, k)
        rel = float((la - lb).detach().double().norm() / lb.detach().double().norm())
        assert rel < 1e-5, (k, rel)
        wk = torch.randn(la.shape, generator=g).to(DEV)
        loss_a, loss_b = loss_a + (la * wk).sum(), loss_b + (lb * wk).sum()
    assert a.latents.inputs._is_empty()
    loss_a.backward()
    loss_b.backward()
    for (n, p), (_, q) in zip(ctp.named_parameters(), ref.named_parameters()):
        rel = float((p.grad - q.grad).double().norm() / (q.grad.double().norm() + 1e-30))
        assert rel < (1e-4 if p.numel() > 16 else 1e-3), (n, rel)
    for (n, x), (_, y) in zip(ctp.named_buffers(), ref.named_buffers()):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-6, msg=n)


class _Loader:
    batch_size = 2

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def _build(ch, seed, dtype, d, hw, pad, alpha=1.0):
    cae = Cae3DCtp(Enc3DCtp(hw, d, ch, 5, alpha, pad, dtype=dtype), Dec3D(hw, d, ch, 5, alpha, dtype=dtype))
    cae.load_state_dict(W.make_state_dict(W.cae_spec(ch), seed))
    return cae.to(DEV)


def _learner(cae, batches, graph=False):
    opt = FusedAdam([p for p in cae.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999),
                    capturable=True)
    learner = CaeReconstructionLearner(_Loader(batches), None, cae, opt, None, n_epochs=1, path_previous_base=None,
                                       path_outputs_base="/tmp/_cae_ctp_test", criterion=BatchDiceLoss([1.0]), verbose=False,
                                       graph=graph, batch_metrics=False)
    return learner, opt


def _batch(seed, d, hw, pad):
    labels, clinical = W.cae_inputs(2, d, hw, seed)
    cbv, ttd = ctp_inputs(seed, d, hw, pad)
    return {"case_id": [0, 1], "images": torch.cat([cbv, ttd], 1), "labels": labels, "clinical": clinical}


def test_matches_reference_fixture(golden_dir):
    """f32 mode against latents / reconstructions / losses / gradient norms / one Adam step of the reference's Cae3DCtp at
    28 x 128 x 128 (the tolerances of test_gpu_cae.py::test_cae_matches_reference_fixture)"""
    fx = np.load(os.path.join(golden_dir, "cae_ctp_200.npz"))
    ch, seed = [int(c) for c in fx["channels"]], int(fx["seed"])
    d, hw, pad = int(fx["d"]), int(fx["hw"]), tuple(int(p) for p in fx["padding"])
    cae = _build(ch, seed, "f32", d, hw, pad, alpha=float(fx["alpha"])).train()
    learner, opt = _learner(cae, [])
    learner.adapt_betas(0)
    assert abs(opt.param_groups[0]["betas"][0] - float(fx["betas_epoch0"][0])) < 1e-12
    dto = learner.inference_step(_batch(seed, d, hw, pad))
    assert dto.latents.inputs._is_empty() and dto.reconstructions.inputs.core is None
    for k in ("core", "penu", "lesion", "interpolation"):
        lat = getattr(dto.latents.gtruth, k).detach().cpu()
        rec = getattr(dto.reconstructions.gtruth, k).detach().cpu()
        np.testing.assert_allclose(lat.reshape(2, -1)[:, :64].numpy(), fx["lat_head/" + k], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(rec[:, 0, d // 2, 60:68, 60:68].numpy(), fx["rec_crop/" + k], rtol=0, atol=2e-4)
    for ep in (0, 30, 60):
        assert abs(float(learner.loss_step(dto, ep)) - float(fx["loss_epoch/%d" % ep])) < 2e-5
    loss = learner.loss_step(dto, 30)
    opt.zero_grad()
    loss.backward()
    for n, p in cae.named_parameters():
        gn = float(fx["gnorm/" + n])
        tol = 5e-3 if p.numel() > 16 else 2e-2
        assert abs(float(p.grad.double().norm()) - gn) <= tol * gn + 1e-9, n
    opt.step()
    for n, p in list(cae.named_parameters())[:8]:
        np.testing.assert_allclose(p.detach().reshape(-1)[:8].cpu().numpy(), fx["phead1/" + n], rtol=1e-3, atol=3e-5)


# ------------------------------------------------------------------------------------------------ training
def _steps(graph, n, seed=17, d=28, hw=64, pad=(2, 4, 4), warmup=1):
    cae = _build(CH, seed, "bf16", d, hw, pad).train()
    batch = _batch(seed, d, hw, pad)
    learner, opt = _learner(cae, [batch], graph=graph)
    learner.GRAPH_WARMUP = warmup
    learner.adapt_betas(0)
    losses = [float(learner.train_batch(batch, 0).loss) for _ in range(n)]
    return losses, [p.detach().clone() for p in cae.parameters()]


def test_captured_steps_follow_the_eager_steps_bit_for_bit():
    """three Learner(graph=True) steps (one eager warm-up, then the captured step) against three eager steps: the same losses,
    bit for bit.  The parameters after the third update differ by a few 1e-6 -- measured the same for the plain Cae3D with the
    same learner and optimiser, i.e. a property of the captured optimiser step, not of the CTP stack input -- and are held to
    1e-5 (a hundredth of the learning rate)."""
    a = _steps(False, 3)
    b = _steps(True, 3)
    assert a[0] == b[0], (a[0], b[0])
    worst = max(float((p - q).abs().max()) for p, q in zip(a[1], b[1]))
    assert worst < 1e-5, worst


def test_loss_falls_over_twenty_steps():
    losses, _ = _steps(False, 20)
    assert all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < losses[0] - 0.01, losses


_CHILD = r"""
import json, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import test_gpu_ctp as T
import stroke_prediction_amd.common.model.Cae3D as M
assert M.CAE_BATCHED == 0
out = {}
cae = T._build(T.CH, 19, "f32", 28, 64, (2, 4, 4)).train()
learner, opt = T._learner(cae, [])
dto = learner.inference_step(T._batch(19, 28, 64, (2, 4, 4)))
loss = learner.loss_step(dto, 30)
opt.zero_grad()
loss.backward()
out["loss"] = float(loss)
out["lat"] = dto.latents.gtruth.lesion.detach().double().reshape(-1)[:256].cpu().tolist()
out["gnorm"] = float(torch.cat([p.grad.reshape(-1) for p in cae.parameters()]).double().norm())
out["graph"] = T._steps(True, 5, warmup=3)[0]      # (pass by pass, the backward's tables are built in the second eager step)
print("RESULT " + json.dumps(out))
"""


def test_pass_by_pass_mode_in_a_child_process():
    """SP_CAE_BATCHED=0: every encoder pass builds its own stack input (G = 1 per launch), concurrently as graph branches
    under capture; f32 results equal the grouped path's, and captured bf16 steps train"""
    env = dict(os.environ, SP_CAE_BATCHED="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads(r.stdout.split("RESULT ", 1)[1].splitlines()[0])
    cae = _build(CH, 19, "f32", 28, 64, (2, 4, 4)).train()
    learner, opt = _learner(cae, [])
    dto = learner.inference_step(_batch(19, 28, 64, (2, 4, 4)))
    loss = learner.loss_step(dto, 30)
    opt.zero_grad()
    loss.backward()
    assert abs(float(loss) - res["loss"]) < 2e-5
    lat = dto.latents.gtruth.lesion.detach().double().reshape(-1)[:256].cpu()
    torch.testing.assert_close(torch.tensor(res["lat"], dtype=torch.float64), lat, rtol=1e-4, atol=1e-5)
    gn = float(torch.cat([p.grad.reshape(-1) for p in cae.parameters()]).double().norm())
    assert abs(gn - res["gnorm"]) <= 2e-3 * gn
    assert all(np.isfinite(res["graph"])) and res["graph"][-1] < res["graph"][0]


# ------------------------------------------------------------------------------------------------ the script
def test_training_script_two_epochs(tmp_path):
    base = str(tmp_path / "cae_ctp")
    env = dict(os.environ, SP_SYNTHETIC_DATA="1", MPLBACKEND="Agg")
    args = ["--epochs", "2", "--batchsize", "2", "--fold", "0", "1", "2", "3", "4", "5", "6", "7",
            "--channelscae", "3", "16", "24", "32", "100", "200", "1", "--padding", "8", "6", "4", "--outbasepath", base]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "stroke-prediction_amd", "train_shape_reconstruction_with_ctp.py")] + args,
                       capture_output=True, text=True, env=env, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Epoch 2/2 training loss" in r.stdout and "Epoch 2/2 validate loss" in r.stdout
    for suffix in ("_cae1.model", "_cae1.optim", "_cae1.json", "_cae1_final.model"):
        assert os.path.exists(base + suffix), suffix
    import re
    losses = [float(v) for v in re.findall(r"training loss: ([0-9.eE+-]+)", r.stdout)]
    assert len(losses) == 2 and all(np.isfinite(losses))
