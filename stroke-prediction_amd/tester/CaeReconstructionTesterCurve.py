"""Per-case curve of Dice / Hausdorff / ASSD of the predicted lesion as the time to treatment is varied (reference
``tester/CaeReconstructionTesterCurve.py:5-42``): the case's own tA->tR, fixed hours, ratios of the case's tA->tR and
fractions of the time to penumbra.  The reference runs the whole model and all three measures once per point; here a case
is one ``inference_curve`` call (encoder once, one decoder call for every point) and the T predictions are measured against
the follow-up lesion by one ``binary_measures_many_torch`` call (``sp_binary_measures_many``).  Lines, their order and their
notes are the reference's."""
import torch

import common.dto.MetricMeasuresDto as MetricMeasuresDtoInit
from common import data, metrics
from tester.CaeReconstructionTester import CaeReconstructionTester

PENUMBRA_FRACTIONS = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]


def curve_schedule(to_to_ta, ta_to_tr, normalization_hours_penumbra, steps_fixed, steps_relative):
    """The ``(step, note)`` points of one case in the reference's order (CaeReconstructionTesterCurve.py:21-42): ``(None, '')`` --
    the case's own time to treatment --, the fixed hours, the ratios of its tA->tR, the fractions of its time to penumbra
    (normalisation - tO->tA).  Pure: the two globals and the settings in, the list out."""
    points = [(None, '')]
    points += [(step, 'ta_to_tr fixed=' + str(step)) for step in steps_fixed]
    points += [(step * ta_to_tr, 'ta_to_tr ratio=' + str(step) + '\t(' + str(step * ta_to_tr) + ')') for step in steps_relative]
    tr_to_penu = normalization_hours_penumbra - to_to_ta
    points += [(step * tr_to_penu, 'tr_to_penumbra=' + str(step) + '\t(' + str(step * tr_to_penu) + ')') for step in PENUMBRA_FRACTIONS]
    return points


class CaeReconstructionTesterCurve(CaeReconstructionTester):
    def __init__(self, dataloader, path_model, path_outputs_base='/tmp/', normalization_hours_penumbra=10,
                 ta_to_tr_fixed_hours=range(11), ta_to_tr_relative_steps=[0, 0.25, 0.5, 0.75, 1, 1.25, 1.5, 1.75, 2]):
        CaeReconstructionTester.__init__(self, dataloader, path_model, path_outputs_base=path_outputs_base,
                                         normalization_hours_penumbra=normalization_hours_penumbra)
        self._steps_fixed = ta_to_tr_fixed_hours
        self._steps_relative = ta_to_tr_relative_steps

    def infer_batch(self, batch: dict, step: float):
        """one point, literally (the reference's method): the whole model and the three measures for this step"""
        with torch.no_grad():
            dto = self.inference_step(batch, step)
        batch_metrics = self.batch_metrics_step(dto)
        return batch_metrics, dto

    def schedule(self, batch: dict):
        g = batch[data.KEY_GLOBAL]
        return curve_schedule(float(g[:, 0].reshape(-1)[0]), float(g[:, 1].reshape(-1)[0]), self._normalization_hours_penumbra,
                              self._steps_fixed, self._steps_relative)

    def infer_curve(self, batch: dict, points):
        """[(batch_metrics, dto)] for the (step, note) points of one case: one model call, three measure calls"""
        with torch.no_grad():
            dtos = self.inference_curve(batch, [step for step, _ in points])
        rec, gt = dtos[0].reconstructions.gtruth, dtos[0].given_variables.gtruth
        core = metrics.binary_measures_torch(rec.core, gt.core, self.is_cuda)          # the same at every point
        penu = metrics.binary_measures_torch(rec.penu, gt.penu, self.is_cuda)
        lesions = metrics.binary_measures_many_torch([d.reconstructions.gtruth.interpolation for d in dtos], gt.lesion, self.is_cuda)
        out = []
        for dto, lesion in zip(dtos, lesions):
            m = MetricMeasuresDtoInit.init_dto()
            m.lesion, m.core, m.penu = lesion, core, penu
            out.append((m, dto))
        return out

    def run_inference(self):
        for batch in self._dataloader:
            points = self.schedule(batch)
            for k, ((batch_metrics, dto), (_, note)) in enumerate(zip(self.infer_curve(batch, points), points)):
                self.print_inference(batch, batch_metrics, dto, note)
                if k == 0:
                    self.save_inference(dto, batch)      # the prediction at the case's own time to treatment
