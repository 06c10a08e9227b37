"""Batch dict -> CaeDto -> model (reference ``common/inference/CaeInference.py:18-69``).

``time_to_treatment = tA->tR / (normalization_hours_penumbra - tO->tA)`` per sample as a
B x 1 x 1 x 1 x 1 float tensor; labels[:, 0..2] are the core / penumbra / follow-up lesion masks.
As in the reference, ``inference_step`` sets ``dto.mode`` (not ``dto.flag``), so the models run
their default branch set."""
import torch

import common.dto.CaeDto as CaeDtoUtil
from common import data
from common.dto.CaeDto import CaeDto
from common.inference.Inference import Inference


class CaeInference(Inference):
    def __init__(self, model, normalization_hours_penumbra=10):
        Inference.__init__(self, model)
        self._normalization_hours_penumbra = normalization_hours_penumbra

    def _device(self):
        return next(self._model.parameters()).device

    def _get_normalization(self, batch):
        to_to_ta = batch[data.KEY_GLOBAL][:, 0].reshape(-1, 1).float()
        return self._normalization_hours_penumbra - to_to_ta

    def get_time_to_treatment(self, batch, global_variables, step):
        normalization = self._get_normalization(batch)
        if step is None:
            ta_to_tr = batch[data.KEY_GLOBAL][:, 1].reshape(-1, 1).float()
            ttt = ta_to_tr / normalization
        else:
            ttt = (step * torch.ones(global_variables.size(0), 1, device=normalization.device)) / normalization
        return ttt.reshape(-1, 1, 1, 1, 1)

    def init_clinical_variables(self, batch: dict, step):
        globals_incl_time = batch[data.KEY_GLOBAL].float()
        n = globals_incl_time.size(0)
        time_to_treatment = self.get_time_to_treatment(batch, globals_incl_time, step)
        dev = self._device() if self.is_cuda else globals_incl_time.device
        # created on the target device: no host->device copy of constants inside the (graph-capturable) step
        type_core = torch.zeros(n, 1, 1, 1, 1, device=dev)
        type_penumbra = torch.ones(n, 1, 1, 1, 1, device=dev)
        if time_to_treatment is not None:        # (CaeStepLearner: the encoder predicts the step)
            time_to_treatment = time_to_treatment.to(dev)
        globals_incl_time = globals_incl_time.to(dev)
        return CaeDtoUtil.init_dto(globals_incl_time, time_to_treatment, type_core, type_penumbra,
                                   None, None, None, None, None)

    def init_gtruth_segm_variables(self, batch: dict, dto: CaeDto):
        labels = batch[data.KEY_LABELS]
        if self.is_cuda:
            labels = labels.to(self._device(), non_blocking=True)
        dto.given_variables.gtruth.core = labels[:, 0:1].float()
        dto.given_variables.gtruth.penu = labels[:, 1:2].float()
        dto.given_variables.gtruth.lesion = labels[:, 2:3].float()
        return dto

    def init_ctp_variables(self, batch: dict, dto: CaeDto):
        """the CT-perfusion maps next to the labels: ``images[:, 0:1]`` (CBV) and ``[:, 1:2]`` (TTD), the modalities of
        train_shape_reconstruction_with_ctp.py in its order, padded as the data pipeline left them.  The reference's
        inference passes None here (CaeInference.py:46-47), so its CTP-conditioned CAE could not run."""
        images = batch[data.KEY_IMAGES]
        if self.is_cuda:
            images = images.to(self._device(), non_blocking=True)
        dto.given_variables.inputs.core = images[:, 0:1].float()
        dto.given_variables.inputs.penu = images[:, 1:2].float()
        return dto

    def infer(self, dto: CaeDto):
        return self._model(dto)

    def inference_step(self, batch: dict, step=None):
        dto = self.init_clinical_variables(batch, step)
        dto.mode = CaeDtoUtil.FLAG_GTRUTH
        dto = self.init_gtruth_segm_variables(batch, dto)
        if getattr(self._model, "USES_CTP_INPUTS", False):       # Cae3DCtp: every other model leaves the inputs alone
            dto = self.init_ctp_variables(batch, dto)
        return self.infer(dto)

    def inference_curve(self, batch: dict, steps):
        """``[inference_step(batch, step) for step in steps]`` (each step a float, or None for the case's own time to treatment) for
        one case at the cost of one: only the interpolated latent differs between the points of a time-to-treatment curve.  The
        encoder runs once, the model's own ``_interpolate`` is applied to the stacked normalised times -- every latent is the value
        the per-step path computes --, and one decoder call reconstructs core, penumbra, lesion and all T interpolations.  Returns
        one ``CaeDto`` per step; the core / penumbra / lesion tensors are shared between them, the interpolations (latents and
        reconstructions) are slices of one tensor.  Batch size 1 and an eval-mode model (the testers' setting: in training
        mode every pass would see batch statistics of its own)."""
        steps = list(steps)
        if not steps:
            return []
        if batch[data.KEY_GLOBAL].size(0) != 1:
            raise ValueError("inference_curve evaluates one case at a time (batch size 1), got %d" % batch[data.KEY_GLOBAL].size(0))
        enc, dec = getattr(self._model, "enc", None), getattr(self._model, "dec", None)
        if enc is None or dec is None or not hasattr(enc, "_interpolate"):
            raise TypeError("inference_curve needs an encoder / decoder model (Cae3D, Cae3DCtp), got %s" % type(self._model).__name__)
        if self._model.training:
            raise RuntimeError("inference_curve evaluates a model in eval mode: call model.eval() first")
        first = self.init_clinical_variables(batch, steps[0])
        g = first.given_variables
        # the normalised times exactly as the per-step path computes them, stacked: (T, 1, 1, 1, 1)
        times = torch.cat([self.get_time_to_treatment(batch, g.globals, s) for s in steps], 0).to(g.globals.device)
        g.time_to_treatment = times[0:1]
        first.mode = CaeDtoUtil.FLAG_GTRUTH
        first = self.init_gtruth_segm_variables(batch, first)
        if getattr(self._model, "USES_CTP_INPUTS", False):
            first = self.init_ctp_variables(batch, first)
        first = enc(first)
        lat = first.latents.gtruth
        lat_intp = enc._interpolate(lat.core, lat.penu, times)                       # (T, C, d, h, w)
        rec_all = dec._run_stack(torch.cat([lat.core, lat.penu, lat.lesion, lat_intp], 0))
        rec_core, rec_penu, rec_lesion, rec_intp = rec_all[0:1], rec_all[1:2], rec_all[2:3], rec_all[3:]
        dtos = []
        for k in range(len(steps)):
            dto = first if k == 0 else CaeDtoUtil.init_dto(g.globals, times[k:k + 1], g.scalar_types.core, g.scalar_types.penu,
                                                           g.inputs.core, g.inputs.penu, g.gtruth.core, g.gtruth.penu, g.gtruth.lesion)
            dto.mode = CaeDtoUtil.FLAG_GTRUTH
            l, r = dto.latents.gtruth, dto.reconstructions.gtruth
            l.core, l.penu, l.lesion, l.interpolation = lat.core, lat.penu, lat.lesion, lat_intp[k:k + 1]
            r.core, r.penu, r.lesion, r.interpolation = rec_core, rec_penu, rec_lesion, rec_intp[k:k + 1]
            dtos.append(dto)
        return dtos
