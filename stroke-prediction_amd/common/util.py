"""Command-line configuration of the reference's scripts (``common/util.py:40-145``): the same parser classes, flag names,
types and defaults -- ``--fold --hemisflipid --validsetsize --seed --xyoriginal --xyresample --zsize --padding --lrsteps``
on every experiment, ``--epochs --batchsize --globals --normalize --inbasepath --outbasepath --steplearning`` for the CAE,
positional ``unetpath`` and ``--channels --epochs --outbasepath`` for the U-Net -- so command lines written for the
reference keep working.  Flags that exist only here are marked (MI355X build).  ``get_vis_samples`` (matplotlib sample
grids, util.py:8-34) belongs to the visualisation hooks, which are no-ops in this build.
"""
import argparse

_UNET_CHANNELS = [2, 16, 32, 64, 32, 16, 32, 2]
_CAE_CHANNELS = [1, 16, 24, 32, 100, 200, 1]

# (flag, keyword arguments) per parser family; the reference declares --xyresample as int with default 0.5 (util.py:50):
# a float is what every caller passes and computes with, so it is parsed as one here
_EXPERIMENT = [
    ("--fold", dict(type=int, nargs="+", default=list(range(29)), help="Fold case indices (internal indices, not case numbers on disk)")),
    ("--hemisflipid", dict(type=float, default=15, help="Case id or greater, at which hemispheric flip is applied")),
    ("--validsetsize", dict(type=float, default=0.5, help="Fraction of validation set size")),
    ("--seed", dict(type=int, default=4, help="Seed for any randomization")),
    ("--xyoriginal", dict(type=int, default=256, help="Original size of slices")),
    ("--xyresample", dict(type=float, default=0.5, help="Factor for resampling slices")),
    ("--zsize", dict(type=int, default=28, help="Number of z slices")),
    ("--padding", dict(type=int, nargs="+", default=[20, 20, 20], help="Padding of patches")),
    ("--lrsteps", dict(type=int, nargs="+", default=[], help="MultiStepLR epochs")),
    # MI355X build
    ("--dtype", dict(type=str, default="bf16", choices=["bf16", "f32"], help="(MI355X build) storage / MFMA precision of the HIP path")),
    ("--graph", dict(action="store_true", default=False, help="(MI355X build) replay each training step as one hipGraph")),
    ("--fusedadam", dict(action="store_true", default=False, help="(MI355X build) FusedAdam on the flat buffers instead of torch.optim.Adam")),
    ("--batchaugment", dict(action="store_true", default=False,
                            help="(MI355X build) CAE training: flip + elastic deformation once per collated batch (data.BatchElasticDeform)")),
    ("--devicecache", dict(action="store_true", default=False,
                           help="(MI355X build) upload every case once and gather each batch from the device-resident cache with one "
                                "kernel launch (data.DeviceCaseCache / CachedBatchLoader)")),
    ("--criterion", dict(type=str, default="dice", choices=["dice", "bce", "dicebce", "boundary", "diceboundary", "tversky", "focaltversky", "focalbce",
                                                                  "tverskyfocalbce"],
                         help="(MI355X build) training criterion (metrics.make_criterion): BatchDiceLoss([1.0]) as the reference, the "
                              "nn.BCELoss() its scripts name as the alternative, their sum, the boundary (signed-distance) loss "
                              "mean(o * phi(t)), Dice + boundary weight * boundary loss, or the class-imbalance criteria: the Tversky "
                              "loss, the focal Tversky loss (gamma 4/3), the focal cross entropy, or Tversky + focal weight * focal "
                              "cross entropy")),
    ("--boundaryweight", dict(type=float, default=0.01,
                              help="(MI355X build) --criterion boundary / diceboundary: weight of the boundary term at epoch 0")),
    ("--boundaryramp", dict(type=float, default=0.0,
                            help="(MI355X build) --criterion boundary / diceboundary: the weight grows by this much per epoch, capped at "
                                 "1.0 (Kervadec et al. use 0.01)")),
    ("--tverskyfp", dict(type=float, default=None,
                         help="(MI355X build) --criterion tversky / focaltversky / tverskyfocalbce: weight of the false positives (default 0.3)")),
    ("--tverskyfn", dict(type=float, default=None,
                         help="(MI355X build) --criterion tversky / focaltversky / tverskyfocalbce: weight of the false negatives (default 0.7)")),
    ("--tverskygamma", dict(type=float, default=None,
                            help="(MI355X build) --criterion tversky / focaltversky / tverskyfocalbce: the loss is (1 - TI)^(1/gamma), gamma >= 1 "
                                 "(default 1, focaltversky 4/3)")),
    ("--focalgamma", dict(type=float, default=None,
                          help="(MI355X build) --criterion focalbce / tverskyfocalbce: the focusing exponent, 0 or >= 1 (default 2)")),
    ("--focalalpha", dict(type=float, default=None,
                          help="(MI355X build) --criterion focalbce / tverskyfocalbce: weight of the foreground voxels in [0, 1] (default 0.25)")),
    ("--focalweight", dict(type=float, default=None,
                           help="(MI355X build) --criterion tverskyfocalbce: weight of the focal cross entropy beside the Tversky term (default 1)")),
    ("--optimizer", dict(type=str, default="adam", choices=["adam", "adamw", "sgd"],
                         help="(MI355X build) optim.make_optimizer: Adam as the reference (torch.optim.Adam, or FusedAdam under --fusedadam / "
                              "--graph / --clipnorm), AdamW (decoupled weight decay) or SGD with momentum (nnU-Net: momentum 0.99, "
                              "Nesterov, poly learning rate, gradients clipped at norm 12); adamw and sgd are always the fused classes")),
    ("--lr", dict(type=float, default=None, help="(MI355X build) learning rate (default 1e-3, --optimizer sgd 1e-2)")),
    ("--momentum", dict(type=float, default=0.99, help="(MI355X build) --optimizer sgd: momentum")),
    ("--nesterov", dict(action=argparse.BooleanOptionalAction, default=True, help="(MI355X build) --optimizer sgd: Nesterov momentum")),
    ("--weightdecay", dict(type=float, default=None, help="(MI355X build) weight decay (default: the script's own 1e-5)")),
    ("--clipnorm", dict(type=float, default=0.0,
                        help="(MI355X build) clip the global gradient norm at this value inside the fused step (clip_grad_norm_ "
                             "semantics, no host read: works under --graph); 0 = off.  With --optimizer adam it selects FusedAdam")),
    ("--lrschedule", dict(type=str, default="multistep", choices=["multistep", "poly"],
                          help="(MI355X build) MultiStepLR at --lrsteps (none without them), or PolynomialLR over --epochs with --lrpower")),
    ("--lrpower", dict(type=float, default=0.9, help="(MI355X build) --lrschedule poly: the exponent")),
]
_CAE = [
    ("--epochs", dict(type=int, default=300, help="Number of epochs")),
    ("--batchsize", dict(type=int, default=4, help="Batch size")),
    ("--globals", dict(type=int, default=5, help="Number of global variables")),
    ("--normalize", dict(type=int, default=10, help="Normalization corresponding to penumbra (hours)")),
    ("--inbasepath", dict(type=str, default=None, help="Path and filename base for loading")),
    ("--outbasepath", dict(type=str, default="/tmp/tmp_out", help="Path and filename base for saving")),
    ("--steplearning", dict(action="store_true", default=False, help="Also learn interpolation step from clinical data")),
]
_UNET = [
    ("unetpath", dict(type=str, help="Path to model of Unet")),
    ("--channels", dict(type=int, nargs="+", default=_UNET_CHANNELS, help="Unet channels")),
    ("--epochs", dict(type=int, default=200, help="Number of epochs")),
    ("--outbasepath", dict(type=str, default="/share/data_zoe1/lucas/Linda_Segmentations/tmp/unet", help="Path and filename base for outputs")),
    # the reference's script reads args.inbasepath and a batch size it hard-codes (train_unet_segmentation.py:12,57): made flags
    ("--inbasepath", dict(type=str, default=None, help="(MI355X build) path and filename base of a training to continue")),
    ("--batchsize", dict(type=int, default=6, help="(MI355X build) batch size (train_unet_segmentation.py:12 hard-codes 6)")),
    ("--patchaugment", dict(action="store_true", default=False,
                            help="(MI355X build) with --devicecache: rotate / scale / elastically deform the training patches and change "
                                 "their intensity inside the kernel that builds the batch (data.PatchAugment, seeded by --seed)")),
    ("--fgfraction", dict(type=float, default=0.0,
                          help="(MI355X build) with --devicecache: share of every training batch whose patch is forced to hold a "
                               "foreground voxel, picked on the device from the cached labels (data.ForegroundOversample, seeded by "
                               "--seed; nnU-Net uses 0.33); 0 = off")),
    ("--fgchannels", dict(type=int, nargs="+", default=None,
                          help="(MI355X build) --fgfraction: the label channels that count as foreground (default: all)")),
    ("--intensityaugment", dict(action="store_true", default=False,
                                help="(MI355X build) blur, noise, brightness, contrast and gamma of every training batch's images on "
                                     "the device (data.IntensityAugment as batch_transform, seeded by --seed; the defaults are nnU-Net's); "
                                     "works with and without --devicecache / --patchaugment / --fgfraction")),
] + [("--ia" + name, dict(type=float, nargs=2, default=list(default), metavar=("LOW", "HIGH"),
                          help="(MI355X build) --intensityaugment: range of the %s" % what))
     for name, default, what in (("noisevariance", (0.0, 0.1), "noise variance (absolute: unit-scale inputs)"),
                                 ("blursigma", (0.5, 1.0), "blur's sigma in voxels"), ("gain", (0.75, 1.25), "brightness factor"),
                                 ("contrast", (0.75, 1.25), "contrast factor"), ("gamma", (0.7, 1.5), "gamma"))
] + [("--iap" + name, dict(type=float, default=default, help="(MI355X build) --intensityaugment: probability per sample of %s" % what))
     for name, default, what in (("noise", 0.1, "noise"), ("blur", 0.2, "blur"), ("blurchannel", 0.5, "blur per channel of a blurred sample"),
                                 ("gain", 0.15, "a brightness change"), ("contrast", 0.15, "a contrast change"), ("gamma", 0.3, "gamma"),
                                 ("gammainvert", 0.1, "the inverted gamma"))
]
_IA_RANGES = ("noisevariance", "blursigma", "gain", "contrast", "gamma")
_IA_PROBS = ("noise", "blur", "blurchannel", "gain", "contrast", "gamma", "gammainvert")


def intensity_augment_kwargs(ns):
    """the ``--ia*`` flags of a parsed U-Net namespace as the keyword arguments of ``data.IntensityAugment``"""
    names = dict(noisevariance="noise_variance", blursigma="blur_sigma", blurchannel="blur_channel", gammainvert="gamma_invert")
    kw = {names.get(n, n): tuple(getattr(ns, "ia" + n)) for n in _IA_RANGES}
    kw.update({"p_" + names.get(n, n): getattr(ns, "iap" + n) for n in _IA_PROBS})
    return kw


_SDM = [
    ("unet", dict(type=str, help="Path to model of Segmentation Unet")),
    ("--channels", dict(type=int, nargs="+", default=_UNET_CHANNELS, help="Unet channels")),
    ("--downsample", dict(type=int, default=1, help="Downsampling to CAE latent representation size")),
    ("--groundtruth", dict(type=int, default=1, help="Use groundtruth instead of UNet segmentations")),
    ("--visualinspection", dict(type=int, default=0, help="Inspect visually before it is saved")),
    ("--outbasepath", dict(type=str, default="/share/data_zoe1/lucas/Linda_Segmentations/tmp/sdm", help="Path and filename base for outputs")),
]


class ExpParser(argparse.ArgumentParser):
    """util.py:40-58; ``parse_args`` prints the namespace like the reference."""
    EXTRA = ()

    def __init__(self):
        super().__init__()
        for flag, kw in list(_EXPERIMENT) + list(self.EXTRA):
            self.add_argument(flag, **kw)

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        print(ns)
        return ns


class CAEParser(ExpParser):
    """The CAE training scripts' chains hold the per-sample ``ElasticDeform``, which cannot run from the device cache: there
    ``--devicecache`` goes with ``--batchaugment`` (the cached whole-volume gather then feeds ``BatchElasticDeform``)."""
    EXTRA = _CAE

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.devicecache and not ns.batchaugment:
            self.error("--devicecache needs --batchaugment here: the per-sample ElasticDeform of the CAE training chain cannot run "
                       "from the device-resident case cache; with both flags the cached gather feeds BatchElasticDeform")
        return ns


class UnetParser(ExpParser):
    """``--patchaugment`` samples the training patches from the device-resident case cache through a per-sample transform: it
    goes with ``--devicecache`` (the per-sample chain has no such path).  So does ``--fgfraction``: the foreground voxel is picked
    from the cached labels.  ``--intensityaugment`` is a batch transform and needs neither; its ``--ia*`` ranges and ``--iap*``
    probabilities are checked whether or not it is given."""
    EXTRA = _UNET

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.patchaugment and not ns.devicecache:
            self.error("--patchaugment needs --devicecache: the augmented patches are sampled from the device-resident case cache "
                       "(sp_patch_sample_batch); the per-sample chain has no such path")
        if not 0 <= ns.fgfraction <= 1:
            self.error("--fgfraction is a share of the batch in [0, 1], got %r" % ns.fgfraction)
        if ns.fgfraction > 0 and not ns.devicecache:
            self.error("--fgfraction needs --devicecache: the foreground voxel is picked from the labels of the device-resident case "
                       "cache (sp_patch_origins_fg); the per-sample chain has no such path")
        for name in _IA_RANGES:
            low, high = getattr(ns, "ia" + name)
            if low > high:
                self.error("--ia%s is LOW HIGH with LOW <= HIGH, got %r %r" % (name, low, high))
            if name == "noisevariance" and low < 0:
                self.error("--ianoisevariance is a variance: it must not be negative, got %r" % low)
            if name != "noisevariance" and not low > 0:
                self.error("--ia%s must be positive (%s <= 0 is no %s), got %r" % (name, name, name, low))
        if int(4.0 * ns.iablursigma[1] + 0.5) > 64:
            self.error("--iablursigma: a sigma of %r needs a blur radius above 64" % ns.iablursigma[1])
        for name in _IA_PROBS:
            if not 0 <= getattr(ns, "iap" + name) <= 1:
                self.error("--iap%s is a probability in [0, 1], got %r" % (name, getattr(ns, "iap" + name)))
        return ns


class SDMParser(ExpParser):
    EXTRA = _SDM


def _with(parser, *more):
    for flag, kw in more:
        parser.add_argument(flag, **kw)
    return parser


_CHANNELSCAE = ("--channelscae", dict(type=int, nargs="+", default=_CAE_CHANNELS, help="CAE channels"))
_CAEPATH = ("caepath", dict(type=str, help="Path to previously trained cae phase1 model"))


def get_args_sdm(argv=None):
    return SDMParser().parse_args(argv)


def get_args_shape_training(argv=None):
    return _with(CAEParser(), _CHANNELSCAE).parse_args(argv)


def get_args_step_training(argv=None):
    return _with(CAEParser(), _CAEPATH, _CHANNELSCAE).parse_args(argv)


def get_args_shape_prediction_training(argv=None):
    return _with(CAEParser(), _CAEPATH,
                 ("--channelsenc", dict(type=int, nargs="+", default=_CAE_CHANNELS, help="CAE channels")),
                 ("--initbycae", dict(action="store_true", default=False, help="Init enc weights by cae's enc"))).parse_args(argv)


def get_args_shape_testing(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--path", action="append", type=str, help="Path to model of Shape CAE")
    p.add_argument("--fold", action="append", type=int, nargs="+", help="Fold case indices")
    p.add_argument("--normalize", type=int, default=10, help="Normalization value corresponding to penumbra (hours)")
    p.add_argument("--outbasepath", type=str, default="/share/data_zoe1/lucas/Linda_Segmentations/tmp/shape", help="Path and filename base for outputs")
    p.add_argument("--xyresample", type=float, default=0.5, help="Factor for resampling slices")
    p.add_argument("--padding", type=int, nargs="+", default=[20, 20, 20], help="Padding of patches")
    return p.parse_args(argv)


def get_args_unet_training(argv=None):
    return UnetParser().parse_args(argv)


def get_vis_samples(train_loader, valid_loader):
    """util.py:8-34 picks six samples for the matplotlib grids of ``visualize_epoch``; those hooks are no-ops here."""
    return [], []
