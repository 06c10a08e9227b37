#!/usr/bin/env python3
"""Phase-1 shape training of the CTP-conditioned CAE on the MI355X path: what the reference's
``train_shape_reconstruction_with_ctp.py:8-69`` sets up -- ``Cae3DCtp(Enc3DCtp, Dec3D)`` trained by ``CaeReconstructionLearner``
with Adam(lr 1e-3, betas (0.99, 0.999), weight decay 1e-5) [+ MultiStepLR] and ``BatchDiceLoss([1.0])`` (``--criterion`` picks another), on the CBV / TTD
modalities padded by ``--padding`` next to the core / penumbra / lesion labels -- with the same flags (``common/util.py``).
The reference script cannot run as written: it passes ``leakage=`` (here ``alpha=0.01``) and its inference never hands the
perfusion maps to the encoder (here ``CaeInference`` does, for models that declare ``USES_CTP_INPUTS``).  Added here:
``--fusedadam``, ``--graph``, ``--dtype``, and synthetic cases when the private data set is absent.  The encoder's first
convolution sees three channels, so ``--channelscae`` starts with 3:

    python stroke-prediction_amd/train_shape_reconstruction_with_ctp.py --epochs 2 --batchsize 4 \\
        --channelscae 3 16 24 32 100 800 1 --fusedadam --graph
"""
import datetime
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stroke_prediction_amd  # noqa: E402,F401
from stroke_prediction_amd import optim  # noqa: E402
from common import data, metrics, util  # noqa: E402
from common.model.Cae3D import Cae3DCtp, Dec3D, Enc3DCtp  # noqa: E402
from learner.CaeReconstructionLearner import CaeReconstructionLearner  # noqa: E402

IMAGE_VOLUMES = ['_CBV_reg1_downsampled', '_TTD_reg1_downsampled']             # CBV, TTD: the encoder's channels 1 and 2
LABEL_VOLUMES = ['_CBVmap_subset_reg1_downsampled', '_TTDmap_subset_reg1_downsampled',
                 '_FUCT_MAP_T_Samplespace_subset_reg1_downsampled']           # core, penumbra, follow-up lesion


def build_model(args):
    side = int(args.xyoriginal * args.xyresample)
    kw = dict(size_input_xy=side, size_input_z=args.zsize, channels=args.channelscae, n_ch_global=args.globals, alpha=0.01,
              dtype=args.dtype)
    # PadImages(px, py, pz) pads the (x, y, z) sample axes; the batch tensors are (B, C, z, y, x), the encoder crops (D, H, W)
    pad = args.padding
    enc = Enc3DCtp(padding=(pad[2], pad[1], pad[0]), **kw)
    return Cae3DCtp(enc, Dec3D(**kw)).cuda()


def build_optimizer(args, cae):
    params = [p for p in cae.parameters() if p.requires_grad]
    print('# optimizing params', sum(p.nelement() for p in params), '/ total: cae', sum(p.nelement() for p in cae.parameters()))
    hyper = dict(lr=1e-3, weight_decay=1e-5, betas=(0.99, 0.999))
    optimizer = optim.make_optimizer(args, params, hyper)      # --optimizer / --clipnorm / --fusedadam / --graph
    return optimizer, optim.make_scheduler(args, optimizer)


def build_loaders(args):
    pad = args.padding
    common = [data.ResamplePlaneXY(args.xyresample), data.HemisphericFlipFixedToCaseId(split_id=args.hemisflipid),
              data.PadImages(pad[0], pad[1], pad[2], pad_value=0)]
    # --batchaugment: the elastic deformation once per collated batch (the case-id flip stays in the chain both loaders share)
    augment = [] if args.batchaugment else [data.ElasticDeform()]
    train_tf = common + augment + [data.ToTensor()]
    valid_tf = common + [data.ToTensor()]
    loaders = data.get_stroke_shape_training_data(IMAGE_VOLUMES, LABEL_VOLUMES, train_tf, valid_tf, args.fold, args.validsetsize,
                                                  seed=args.seed, batchsize=args.batchsize,
                                                  batch_transform=data.BatchElasticDeform() if args.batchaugment else None,
                                                  device_cache=args.devicecache)
    print('Size training set:', len(loaders[0].sampler.indices), 'samples | Size validation set:', len(loaders[1].sampler.indices),
          'samples | Capacity batch:', args.batchsize, 'samples')
    return loaders


def train(args):
    if len(args.padding) != 3:
        raise SystemExit("--padding takes three values (x y z)")
    cae = build_model(args)
    optimizer, scheduler = build_optimizer(args, cae)
    ds_train, ds_valid = build_loaders(args)
    criterion = metrics.make_criterion(args.criterion)
    metrics.configure_criterion(criterion, args)      # --boundaryweight / --boundaryramp; nothing for the other criteria
    learner = CaeReconstructionLearner(ds_train, ds_valid, cae, optimizer, scheduler, n_epochs=args.epochs,
                                       path_previous_base=args.inbasepath, path_outputs_base=args.outbasepath,
                                       criterion=criterion, normalization_hours_penumbra=args.normalize,
                                       graph=args.graph)
    learner.run_training()
    return learner


if __name__ == '__main__':
    print(datetime.datetime.now())
    train(util.get_args_shape_training())
    print(datetime.datetime.now())
