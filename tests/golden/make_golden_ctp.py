#!/usr/bin/env python3
"""Generate ``cae_ctp_200.npz`` by running the REAL reference ``Cae3DCtp(Enc3DCtp, Dec3D)`` on CPU (modelled on ``gen_cae`` in
``make_golden.py``; same environment, no test runs this file):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_ctp.py

The reference's inference leaves the CTP inputs ``None`` (CaeInference.py:46-47), so the DTO is completed by hand: the
reference learner's ``init_clinical_variables`` / ``init_gtruth_segm_variables``, then ``given_variables.inputs`` = the padded
CBV / TTD volumes of ``ctp_inputs`` below (deterministic from ``oracle.weights``; tests/test_gpu_ctp.py rebuilds them the same
way), then the reference's ``infer`` / ``loss_step`` / backward / Adam step.  Recorded: the keys of ``cae_200.npz``.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _FakeLoader, digest, grads_summary, import_reference  # noqa: E402

CH = (3, 16, 24, 32, 100, 200, 1)
PADDING = (2, 8, 8)          # D, H, W voxels per side
ALPHA = 1.0                  # ELU(1) is C1: gradient norms stay smooth across the tolerance (as in cae_200.npz)


def ctp_inputs(seed, d, hw, padding):
    """padded CBV / TTD volumes (2, 1, d + 2 pD, hw + 2 pH, hw + 2 pW) in (0.05, 0.95): blobs of another seed, zero outside"""
    from oracle import weights as W
    seg, _ = W.cae_inputs(2, d, hw, seed + 11)
    cbv = 0.05 + 0.6 * seg[:, 0:1] + 0.3 * seg[:, 2:3]
    ttd = 0.05 + 0.9 * seg[:, 1:2]
    pd, ph, pw = padding
    pad = lambda t: torch.nn.functional.pad(t, (pw, pw, ph, ph, pd, pd)).contiguous()
    return pad(cbv), pad(ttd)


def gen_cae_ctp(seed, fname, ch=CH, d=28, hw=128, padding=PADDING):
    from oracle import weights as W
    from common.model.Cae3D import Cae3DCtp, Enc3DCtp, Dec3D
    from common.metrics import BatchDiceLoss
    from learner.CaeReconstructionLearner import CaeReconstructionLearner
    ch = list(ch)
    enc = Enc3DCtp(size_input_xy=hw, size_input_z=d, channels=ch, n_ch_global=5, alpha=ALPHA, padding=padding)
    dec = Dec3D(size_input_xy=hw, size_input_z=d, channels=ch, n_ch_global=5, alpha=ALPHA)
    cae = Cae3DCtp(enc, dec)
    cae.load_state_dict(W.make_state_dict(W.cae_spec(ch), seed))
    params = [p for p in cae.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    learner = CaeReconstructionLearner(_FakeLoader(), None, cae, opt, None, n_epochs=1, path_previous_base=None,
                                       path_outputs_base="/tmp/_golden_cae_ctp", criterion=BatchDiceLoss([1.0]))
    labels, clinical = W.cae_inputs(2, d, hw, seed)
    cbv, ttd = ctp_inputs(seed, d, hw, padding)
    batch = {"case_id": [0, 1], "images": torch.cat([cbv, ttd], 1), "labels": labels, "clinical": clinical}
    fx = {"channels": np.array(ch), "seed": np.array(seed), "d": np.array(d), "hw": np.array(hw),
          "padding": np.array(padding), "alpha": np.array(ALPHA), "torch_version": np.array(torch.__version__)}
    cae.train()
    learner.adapt_betas(0)
    fx["betas_epoch0"] = np.array(opt.param_groups[0]["betas"])
    dto = learner.init_clinical_variables(batch, None)
    dto = learner.init_gtruth_segm_variables(batch, dto)
    dto.given_variables.inputs.core, dto.given_variables.inputs.penu = cbv, ttd
    dto = learner.infer(dto)
    assert dto.latents.inputs._is_empty() and dto.reconstructions.inputs.core is None
    fx["ttt"] = dto.given_variables.time_to_treatment.detach().numpy().copy()
    for k in ("core", "penu", "lesion", "interpolation"):
        lat = getattr(dto.latents.gtruth, k)
        rec = getattr(dto.reconstructions.gtruth, k)
        fx["lat_digest/" + k] = digest(lat)
        fx["lat_head/" + k] = lat.detach().reshape(lat.shape[0], -1)[:, :64].numpy().copy()
        fx["rec_digest/" + k] = digest(rec)
        fx["rec_crop/" + k] = rec.detach()[:, 0, d // 2, 60:68, 60:68].numpy().copy()
    for ep in (0, 30, 60):
        fx["loss_epoch/%d" % ep] = np.float64(learner.loss_step(dto, ep).item())
    loss = learner.loss_step(dto, 30)
    opt.zero_grad()
    loss.backward()
    fx.update(grads_summary(cae.named_parameters()))
    opt.step()
    for n, b in cae.named_buffers():
        if n.endswith("num_batches_tracked"):
            fx["nbt/" + n] = b.numpy().copy()
        elif n.startswith("enc.encoder.0.") or n.startswith("dec.decoder.0.") or n.startswith("dec.decoder.33."):
            fx["buf1/" + n] = b.detach().numpy().copy()
    for n, p in list(cae.named_parameters())[:8]:
        fx["phead1/" + n] = p.detach().reshape(-1)[:8].numpy().copy()
    np.savez_compressed(os.path.join(HERE, fname), **fx)
    print("\nwrote", fname, {k: float(v) for k, v in fx.items() if k.startswith("loss_epoch")})


if __name__ == "__main__":
    import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    gen_cae_ctp(31, "cae_ctp_200.npz")
