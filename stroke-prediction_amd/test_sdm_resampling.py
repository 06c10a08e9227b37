#!/usr/bin/env python3
"""The signed-distance-map (SDM) interpolation baseline of the reference (``test_sdm_resampling.py``), which the reference's
README offers for comparison with the CAE, on the MI355X path.  Same command line (``common/util.py`` ``get_args_sdm``), same
transforms and test-data call, same per-case line and results line; the fields, the measures and the exports are computed on
the device (``common/sdm.py``, ``csrc/sp_sdm.hip``).  Synthetic cases stand in when the private data set is absent:

    python stroke-prediction_amd/test_sdm_resampling.py x.model --fold 0 1 --outbasepath /tmp/sdm/sdm

Differences from the reference: the results line goes to ``<dirname(--outbasepath)>/sdm_results.txt`` (the reference
hard-codes the directory of its default ``--outbasepath``); the four volumes are written as
``<outbasepath>_<case>_{lesion,fuctgt,core,penu}.npy`` (NIfTI writing is out of scope, as in ``CaeReconstructionTester``);
``--visualinspection`` is a no-op like the other visualisation hooks.  The file keeps the reference's name and defines no
tests.
"""
import datetime
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stroke_prediction_amd  # noqa: E402,F401
from common import data, metrics, util  # noqa: E402
from common.sdm import sdm_interpolate_numpy, sdm_interpolate_torch, zoom_torch  # noqa: E402,F401

NORMALIZATION_HOURS_PENUMBRA = 10
MODALITIES = ['_unet_core', '_unet_penu']
LABELS = ['_CBVmap_subset_reg1_downsampled', '_TTDmap_subset_reg1_downsampled', '_FUCT_MAP_T_Samplespace_subset_reg1_downsampled']
RESULT_LINE = 'Evaluate case: {} - DC:{:.3}, HD:{:.3}, ASSD:{:.3}, Core recon DC:{:.3}, Penu recon DC:{:.3}'


def get_normalized_time(batch, normalization_hours_penumbra):
    """(tO->tA as a float32 CPU tensor (B, 1, 1, 1, 1), normalization = hours - tO->tA as float32 (B, 1)): the reference's
    float32 operations in its order.  (B, 1) comes from a reshape, so a batch of one works as it did under torch 0.3."""
    to_to_ta = batch[data.KEY_GLOBAL][:, 0, :, :, :].unsqueeze(data.DIM_CHANNEL_TORCH3D_5).type(torch.FloatTensor)
    normalization = torch.ones(to_to_ta.size()[0], 1).type(torch.FloatTensor) * normalization_hours_penumbra - \
        to_to_ta.reshape(-1, 1)
    return to_to_ta, normalization


def time_to_treatment(batch, normalization):
    """tA->tR / normalization in float32 (reference test_sdm_resampling.py:110-111)"""
    ta_to_tr = batch[data.KEY_GLOBAL][:, 1, :, :, :].reshape(-1, 1)
    return ta_to_tr.type(torch.FloatTensor) / normalization


def _export(path, volume):
    """(D, H, W) device volume -> the reference's (x, y, z) orientation, written as .npy"""
    np.save(path, volume.cpu().numpy().transpose((2, 1, 0)))


def infer(args=None):
    args = util.get_args_sdm(args)
    print('Evaluate validation set', args.fold)
    transform = [data.ResamplePlaneXY(args.xyresample),
                 data.HemisphericFlipFixedToCaseId(split_id=args.hemisflipid),
                 data.ToTensor()]
    ds_test = data.get_testdata(modalities=MODALITIES, labels=LABELS, transform=transform, indices=args.fold)
    out_dir = os.path.dirname(args.outbasepath)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    results_path = os.path.join(out_dir, 'sdm_results.txt')

    for sample in ds_test:
        case_id = sample[data.KEY_CASE_ID].cpu().numpy()[0]
        _, normalization = get_normalized_time(sample, NORMALIZATION_HOURS_PENUMBRA)
        ttt = time_to_treatment(sample, normalization)
        labels = sample[data.KEY_LABELS].cuda()
        lesion = labels[:, 2:3]
        source = labels if args.groundtruth else sample[data.KEY_IMAGES].cuda()
        core, penu = source[:, 0:1], source[:, 1:2]

        recon_core, recon_intp, recon_penu, _, _, _, (m_intp, m_core, m_penu) = sdm_interpolate_torch(
            core, penu, ttt.reshape(()), threshold=0.5, zoom=12, resample=args.downsample, masks=True)

        print(int(sample[data.KEY_CASE_ID]), 'TO-->TR', float(ttt))

        results = metrics.binary_measures_torch(m_intp, lesion[0, 0].float(), True, binary_threshold=0.5)
        c_res = metrics.binary_measures_torch(m_core, core[0, 0].float(), True, binary_threshold=0.5)
        p_res = metrics.binary_measures_torch(m_penu, penu[0, 0].float(), True, binary_threshold=0.5)
        with open(results_path, 'a') as f:
            print(RESULT_LINE.format(case_id, results.dc, results.hd, results.assd, c_res.dc, p_res.dc), file=f)

        base = args.outbasepath + '_' + str(case_id)
        _export(base + '_lesion.npy', zoom_torch(recon_intp, (1, 2, 2), out="gt0"))
        _export(base + '_fuctgt.npy', zoom_torch(lesion[0, 0].float(), (1, 2, 2), out="i8", src_as_int8=True))
        _export(base + '_core.npy', zoom_torch(recon_core, (1, 2, 2), out="lt0"))
        _export(base + '_penu.npy', zoom_torch(recon_penu, (1, 2, 2), out="gt0"))
        del sample


if __name__ == '__main__':
    print(datetime.datetime.now())
    infer()
    print(datetime.datetime.now())
