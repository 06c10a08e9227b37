#!/usr/bin/env python3
"""Per-case evaluation of trained shape CAEs on the MI355X path (the reference's ``test_shape_reconstruction.py``): one
``--path MODEL --fold I J ...`` pair per fold; every case of a fold goes through ``CaeReconstructionTester`` -- the
predicted lesion at the case's own time to treatment, measured against the follow-up lesion -- and prints one line.
Synthetic cases stand in when the private data set is absent:

    python stroke-prediction_amd/test_shape_reconstruction.py --path /tmp/tmp_out_cae1.model --fold 0 1 --padding 0 0 0 --outbasepath /tmp/shape/eval

Differences from the reference: the reconstructions are written as ``<outbasepath>_<case>_{core,pred,penu}.npy`` (NIfTI
writing is out of scope, as in the testers); the model is moved to the GPU after loading.  The file keeps the
reference's name and defines no tests.
"""
import datetime
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stroke_prediction_amd  # noqa: E402,F401
from common import data, util  # noqa: E402
from tester.CaeReconstructionTester import CaeReconstructionTester  # noqa: E402

IMAGE_VOLUMES = ['_CBV_reg1_downsampled', '_TTD_reg1_downsampled']
LABEL_VOLUMES = ['_CBVmap_subset_reg1_downsampled', '_TTDmap_subset_reg1_downsampled',
                 '_FUCT_MAP_T_Samplespace_subset_reg1_downsampled']          # core, penumbra, follow-up lesion


def fold_loaders(args):
    """(model path, test loader) per --path / --fold pair, in the order given"""
    assert args.path and args.fold and len(args.fold) == len(args.path), \
        'You must provide as many --fold arguments as --path model arguments, in the exact same order!'
    out_dir = os.path.dirname(args.outbasepath)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    pad = args.padding
    for k, (path, fold) in enumerate(zip(args.path, args.fold)):
        transform = [data.ResamplePlaneXY(args.xyresample), data.PadImages(pad[0], pad[1], pad[2], pad_value=0), data.ToTensor()]
        loader = data.get_testdata(modalities=IMAGE_VOLUMES, labels=LABEL_VOLUMES, transform=transform, indices=fold)
        print('Model ' + path + ' of fold ' + str(k + 1) + '/' + str(len(args.fold)) + ' with indices: ' + str(fold))
        print('Size test set:', len(loader.sampler.indices), '| # batches:', len(loader))
        yield path, loader


def load_model(path):
    return torch.load(path, weights_only=False).cuda()


def evaluate(args):
    for path, loader in fold_loaders(args):
        CaeReconstructionTester(loader, load_model(path), args.outbasepath, args.normalize).run_inference()


if __name__ == '__main__':
    print(datetime.datetime.now())
    evaluate(util.get_args_shape_testing())
    print(datetime.datetime.now())
