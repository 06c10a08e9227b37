#!/usr/bin/env python3
"""Per-case evaluation of a trained segmentation U-Net on the MI355X path (the reference's ``test_unet_segmentation.py``):
the network was trained on patches, but is fully convolutional -- every case of ``--fold`` goes through it as one whole
volume, padded by ``--padding`` (20 20 20: what the valid convolutions take off again), and prints its core / penumbra Dice.
Synthetic cases stand in when the private data set is absent:

    python stroke-prediction_amd/test_unet_segmentation.py /tmp/unet.model --fold 0 1 --outbasepath /tmp/unet/eval

Differences from the reference: the probability maps are written as ``<outbasepath>_<case>_{core,penu}.npy`` (NIfTI writing
is out of scope, as in the testers); the model is moved to the GPU after loading.  The file keeps the reference's name and
defines no tests.
"""
import datetime
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stroke_prediction_amd  # noqa: E402,F401
from common import data, util  # noqa: E402
from common.model.Unet3D import Unet3D  # noqa: E402,F401  (the pickled model's class)
from tester.UnetSegmentationTester import UnetSegmentationTester  # noqa: E402

IMAGE_VOLUMES = ['_CBV_reg1_downsampled', '_TTD_reg1_downsampled']
LABEL_VOLUMES = ['_CBVmap_subset_reg1_downsampled', '_TTDmap_subset_reg1_downsampled']     # core, penumbra


def evaluate(args):
    pad = args.padding
    transform = [data.ResamplePlaneXY(args.xyresample), data.PadImages(pad[0], pad[1], pad[2], pad_value=0), data.ToTensor()]
    loader = data.get_testdata(modalities=IMAGE_VOLUMES, labels=LABEL_VOLUMES, transform=transform, indices=args.fold)
    print('Size test set:', len(loader.sampler.indices), '| # batches:', len(loader))
    out_dir = os.path.dirname(args.outbasepath)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    model = torch.load(args.unetpath, weights_only=False).cuda()
    UnetSegmentationTester(loader, model, args.outbasepath, None).run_inference()


if __name__ == '__main__':
    print(datetime.datetime.now())
    evaluate(util.get_args_unet_training())
    print(datetime.datetime.now())
