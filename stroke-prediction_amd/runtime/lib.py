"""ctypes binding of ``libstroke_amd.so``, derived from the one definition of its C ABI, ``include/stroke_amd.h``.

The header is read once at import (``parse_header``): every ``typedef struct`` becomes a ``ctypes.Structure``, every declared
function gets its ``argtypes`` / ``restype``, every ``enum`` constant its value.  An entry point added to the header and to a
``.hip`` file is callable with no edit here; a declaration the parser does not understand raises at import.

The library is built in-tree by ``__graft_entry__.build()`` (``hipcc
--offload-arch=gfx950``).  There is no fallback: if it is missing or a call
fails, a ``RuntimeError`` carrying ``sp_last_error`` is raised.
"""
import ctypes as C
import os
import re
import threading as _threading

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(_HERE)
LIB_PATH = os.environ.get("SP_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libstroke_amd.so")   # SP_LIB_PATH: diagnostic builds (tools/)
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
HEADER = os.path.join(os.path.dirname(PKG_DIR), "include", "stroke_amd.h")
SOURCES = ["sp_conv.hip", "sp_conv_dma.hip", "sp_conv_par.hip", "sp_conv_zm.hip", "sp_conv_zm8.hip", "sp_wgrad.hip", "sp_wgrad_dma.hip", "sp_conv_fc.hip", "sp_wgrad_zr.hip", "sp_wgrad_pw.hip", "sp_wgrad_f8.hip", "sp_plan.hip", "sp_comm.hip", "sp_head.hip", "sp_first.hip", "sp_elem.hip", "sp_pwout.hip",
           "sp_transform.hip", "sp_augment.hip", "sp_intensity.hip", "sp_gather.hip", "sp_fgpatch.hip", "sp_sample.hip", "sp_ctp.hip", "sp_sdm.hip", "sp_boundary.hip", "sp_loss.hip", "sp_optim.hip"]

i32, i64, f32, f64, vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p
_POINTEES = {"void", "char", "unsigned long long"}      # what the header names behind a `*` only
_STATEMENT = re.compile(r"\s*((?:[^;{}]|\{[^{}]*\})+?)\s*;")      # up to the next `;` outside braces


def parse_header(text):
    """The declarations of a C header written like ``stroke_amd.h`` -> (structs, sigs, consts): a ``ctypes.Structure`` per struct
    typedef, ``(argtypes, restype)`` per function, the value per enum constant.  ``int`` / ``int32_t`` -> ``c_int32``, ``int64_t``,
    ``float``, ``double``, ``size_t`` -> their ctypes, every pointer -> ``c_void_p`` (which takes ``byref(...)``, ctypes arrays, raw
    device addresses and ``None``).  Comments and preprocessor lines are dropped; what remains must be typedefs of structs or of
    known types, anonymous enums of ``NAME = integer`` entries and function declarations: anything else raises ``ValueError``
    with the offending text."""
    types = {"int": i32, "int32_t": i32, "int64_t": i64, "float": f32, "double": f64, "size_t": C.c_size_t}
    structs, sigs, consts = {}, {}, {}

    def fail(what, decl):
        raise ValueError("stroke_amd.h: %s in `%s`" % (what, " ".join(decl.split())[:160]))

    def ctype(spec, decl):           # "const float*" -> c_void_p, "int32_t" -> c_int32, "sp_bn_bwd_args" -> that Structure
        spec = re.sub(r"\bconst\b", " ", spec)
        base = " ".join(spec.replace("*", " ").split())
        if base not in types and not ("*" in spec and base in _POINTEES):
            fail("unknown type `%s`" % base, decl)
        return vp if "*" in spec else types[base]

    def declarator(item, decl):      # "const float* gamma" -> ("const float*", "gamma")
        m = re.fullmatch(r"\s*([^()]*[\s*])(\w+)\s*", item)
        return m.groups() if m else fail("no `type name` in `%s`" % item.strip(), decl)

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)      # extern "C" { and its }
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    pos = 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            fail("unterminated declaration", text[pos:])
        decl, pos = m.group(1), m.end()
        if (m := re.fullmatch(r"typedef\s+struct\s+\w*\s*\{(.*)\}\s*(\w+)", decl, re.S)):
            fields = []
            for member in filter(str.strip, m.group(1).split(";")):
                first, *more = member.split(",")                   # "int32_t B, Di, Hi": one type, three fields
                spec, name = declarator(first, decl)
                if not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
                    fail("declarators of `%s`" % member.strip(), decl)
                fields += [(n.strip(), ctype(spec, decl)) for n in [name] + more]
            types[m.group(2)] = structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})
        elif (m := re.fullmatch(r"typedef\s(.*)", decl, re.S)):
            spec, name = declarator(m.group(1), decl)
            types[name] = ctype(spec, decl)
        elif (m := re.fullmatch(r"enum\s*\{(.*)\}", decl, re.S)):
            for entry in filter(str.strip, m.group(1).split(",")):
                e = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", entry) or fail("enum entry `%s` is not NAME = integer" % entry.strip(), decl)
                consts[e.group(1)] = int(e.group(2))
        elif (m := re.fullmatch(r"([^()]*)\(([^()]*)\)", decl, re.S)):
            ret, name = declarator(m.group(1), decl)
            params = [] if m.group(2).strip() == "void" else m.group(2).split(",")
            sigs[name] = ([ctype(declarator(p, decl)[0], decl) for p in params], None if ret.strip() == "void" else ctype(ret, decl))
        else:
            fail("neither typedef, enum nor function", decl)
    return structs, sigs, consts


with open(HEADER) as _f:
    STRUCTS, SIGS, CONSTS = parse_header(_f.read())
EXPORTS = sorted(SIGS)
BnFinArgs, BnBwdArgs, ConvArgs, WgradArgs, WgradF8Args, ConvFcArgs, Conv3dDesc, Conv3dPlan, Conv3dWgradPlan, PrepItem, F8PrepItem = (
    STRUCTS[n] for n in ("sp_bn_fin_args", "sp_bn_bwd_args", "sp_conv_args", "sp_wgrad_args", "sp_wgrad_f8_args", "sp_conv_fc_args",
                         "sp_conv3d_desc", "sp_conv3d_plan_t", "sp_conv3d_wgrad_plan_t", "sp_prep_item", "sp_f8_prep_item"))
# SP_HL: bf16 pair (hi + lo tensors), the forward storage of the "bf16x3" mode; SP_REDUCE_ROWS: replica rows of the accumulators
# the elementwise kernels reduce into
SP_BF16, SP_F32, SP_HL, SP_REDUCE_ROWS = (CONSTS[n] for n in ("SP_BF16", "SP_F32", "SP_HL", "SP_REDUCE_ROWS"))
ACT_NONE, ACT_LEAKY, ACT_ELU, ACT_SIGMOID = (CONSTS["SP_ACT_" + n] for n in ("NONE", "LEAKY", "ELU", "SIGMOID"))
SP_VLOSS_DICE, SP_VLOSS_BCE = CONSTS["SP_VLOSS_DICE"], CONSTS["SP_VLOSS_BCE"]      # the terms of the sp_vloss_* / sp_cae_loss_crit_* calls
SP_TLOSS_TVERSKY, SP_TLOSS_FOCAL = CONSTS["SP_TLOSS_TVERSKY"], CONSTS["SP_TLOSS_FOCAL"]      # the terms of the sp_tloss_* calls


def SP_VLOSS_PITCH(C):
    """row pitch (doubles) of the sp_vloss_* accumulator: the header's macro of that name (the parser drops preprocessor lines)"""
    return (4 * C + 15) // 16 * 16


def SP_BLOSS_PITCH(C):
    """row pitch (doubles) of the sp_bloss_* accumulator: the header's SP_BLOSS_PITCH = SP_VLOSS_PITCH"""
    return SP_VLOSS_PITCH(C)


def SP_TLOSS_PITCH(C):
    """row pitch (doubles) of the sp_tloss_* accumulator: the header's SP_TLOSS_PITCH = SP_VLOSS_PITCH"""
    return SP_VLOSS_PITCH(C)


# precision modes of the models (``Unet3D(dtype=...)``, ``Enc3D(dtype=...)``) -> storage type of the engine's tensors
DTYPE_CODES = {"bf16": SP_BF16, "f32": SP_F32, "fp8": SP_BF16, "fp8b": SP_BF16, "f16": SP_BF16, "bf16x3": SP_BF16, "f16x3": SP_BF16}
#   fp8: bf16 storage + fp8 MFMA operands (runtime/f8.py); fp8b: the bf16 forward with the fp8 BACKWARD (data and weight
#   gradients on e5m2 / e4m3 operands) -- the forward, and with it the direction of the gradients, is the bf16 mode's; f16: IEEE-half storage -- the SAME sources built with
#   -DSP_HALF_F16 into libstroke_amd_f16.so (csrc/sp_common.h), selected per engine with ``use("f16")``; the kernels'
#   dtype code stays SP_BF16 = "the 16-bit storage type of this library";
#   bf16x3: the FORWARD activations are bf16 pairs (hi + lo tensors, SP_HL: ~17 bits; three MFMAs per product), the backward
#   pass is the bf16 one on the hi tensors -- logits within 1e-3 of the fp32 reference at ~1.5x the bf16 step;
#   f16x3: the same in the IEEE-half build (pairs of halves: ~22 bits forward; the backward is the f16 mode's, 8x closer than bf16)
VARIANTS = {"": ("libstroke_amd.so", []), "f16": ("libstroke_amd_f16.so", ["-DSP_HALF_F16"])}
VARIANT_OF = {"bf16": "", "f32": "", "fp8": "", "fp8b": "", "f16": "f16", "bf16x3": "", "f16x3": "f16"}

_libs = {}
_tls = _threading.local()


def current_variant():
    return getattr(_tls, "variant", "")


class use:
    """``with use("f16"):`` -- calls made by this thread inside the block go to that build of the library (an engine is bound
    to one build: its tensors hold that build's 16-bit format)."""

    def __init__(self, variant):
        self.variant = variant or ""

    def __enter__(self):
        self.prev = current_variant()
        _tls.variant = self.variant
        return self

    def __exit__(self, *exc):
        _tls.variant = self.prev
        return False


def lib_path(variant=""):
    if variant == "":
        return LIB_PATH
    return os.path.join(os.path.dirname(LIB_PATH), VARIANTS[variant][0])


def load(variant=None):
    """Load the shared library (of the calling thread's current build, or the named one) once; raises if it has not been built."""
    variant = current_variant() if variant is None else variant
    lib = _libs.get(variant)
    if lib is None:
        # torch bundles its own HIP runtime (libamdhip64): import it FIRST so that this library binds to the
        # same runtime instance (streams and device pointers are shared with torch); loading ours first would
        # pull a second copy from /opt/rocm that never sees torch's context.
        import torch  # noqa: F401
        path = lib_path(variant)
        if not os.path.exists(path):
            raise RuntimeError(
                "stroke_prediction_amd: %s is missing -- build it with `python -c \"import __graft_entry__ as g; "
                "g.build()\"` (hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback." % path)
        lib = C.CDLL(path)
        for name, (argtypes, restype) in SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _libs[variant] = lib
    return lib


def last_error():
    buf = C.create_string_buffer(512)
    load().sp_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, last_error()))


def call(name, *args):
    """Call an ``int sp_*(...)`` entry point and raise on a non-zero return."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d): %s" % (name, rc, last_error()))


def build(verbose=False):
    """Compile the HIP sources for gfx950 into ``lib/libstroke_amd.so`` and its precision variants (cross-compiles without a
    GPU).  One object per source and build (rebuilt only when stale, all compiled concurrently), then one link per build."""
    import subprocess
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    srcs = [os.path.join(CSRC_DIR, s) for s in SOURCES]
    hdrs = [os.path.join(CSRC_DIR, "sp_common.h"), os.path.join(CSRC_DIR, "sp_edt.h"), os.path.join(CSRC_DIR, "sp_gauss.h"),
            os.path.join(CSRC_DIR, "sp_philox.h"), HEADER]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs, links = [], []
    for variant, (fname, flags) in VARIANTS.items():
        if os.environ.get("SP_LIB_PATH"):
            # a diagnostic build named by the environment (tools/build_variant*.sh, tools/build_asan.sh) is used as it is: nothing is
            # compiled beside it (the precision variants would land in ITS directory: six minutes of hipcc inside the sanitizer run)
            break
        out = lib_path(variant)
        if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in srcs + hdrs):
            continue
        objdir = os.path.join(os.path.dirname(LIB_PATH), "obj" + ("_" + variant if variant else ""))
        os.makedirs(objdir, exist_ok=True)
        objs = []
        for src in srcs:
            obj = os.path.join(objdir, os.path.basename(src) + ".o")
            objs.append(obj)
            if not (os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in [src] + hdrs)):
                cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + flags + ["-c", src, "-o", obj]
                if verbose:
                    print(" ".join(cmd))
                jobs.append((cmd, subprocess.Popen(cmd)))
        links.append([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-ldl"])
    for cmd, pr in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    for cmd in links:
        subprocess.run(cmd, check=True)
    if links:
        _libs.clear()
    return LIB_PATH
