#!/usr/bin/env python3
"""The time-to-treatment curve of trained shape CAEs on the MI355X path (the reference's
``test_shape_reconstruction_CurveAnalysis.py``): per case 27 lines -- its own tA->tR, the fixed hours 0 .. 5, nine ratios of
its tA->tR, eleven fractions of its time to penumbra -- with Dice / Hausdorff / ASSD of the predicted lesion at each point.
A case costs one model call and one batched measures call (``tester/CaeReconstructionTesterCurve.py``).  Same command line
and conventions as ``test_shape_reconstruction.py``:

    python stroke-prediction_amd/test_shape_reconstruction_CurveAnalysis.py --path /tmp/tmp_out_cae1.model --fold 0 1 --padding 0 0 0 --outbasepath /tmp/shape/curve

The file keeps the reference's name and defines no tests.
"""
import datetime
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stroke_prediction_amd  # noqa: E402,F401
from common import util  # noqa: E402
from tester.CaeReconstructionTesterCurve import CaeReconstructionTesterCurve  # noqa: E402
from test_shape_reconstruction import fold_loaders, load_model  # noqa: E402

FIXED_HOURS = range(6)      # tA->tR of 0 .. 5 hours


def evaluate(args):
    for path, loader in fold_loaders(args):
        CaeReconstructionTesterCurve(loader, load_model(path), args.outbasepath, args.normalize, FIXED_HOURS).run_inference()


if __name__ == '__main__':
    print(datetime.datetime.now())
    evaluate(util.get_args_shape_testing())
    print(datetime.datetime.now())
