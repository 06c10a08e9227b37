"""The C-ABI library loads on a CPU-only box and exports every symbol include/stroke_amd.h declares."""
import ctypes
import os
import re

from stroke_prediction_amd.runtime import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "stroke_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    names = _declared()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), "missing export %s" % n
    assert sorted(names) == L.EXPORTS, (sorted(set(names) ^ set(L.EXPORTS)))


def test_derived_struct_layouts_match_the_c_compiler(tmp_path):
    """runtime/lib.py derives its ctypes structures from the header; the C compiler is the authority on padding: every sizeof and
    every field offset of the derived classes, nested members included, holds as a _Static_assert against stroke_amd.h"""
    import subprocess
    assert sorted(L.STRUCTS) == sorted(re.findall(r"\}\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", open(L.HEADER).read(), flags=re.S))) and len(L.STRUCTS) == 11
    lines = ['#include "stroke_amd.h"']
    for cname, T in L.STRUCTS.items():
        lines.append("_Static_assert(sizeof(%s) == %d, \"sizeof %s\");" % (cname, ctypes.sizeof(T), cname))
        for field, _ in T._fields_:
            lines.append("_Static_assert(offsetof(%s, %s) == %d, \"%s.%s\");" % (cname, field, getattr(T, field).offset, cname, field))
    assert len(lines) > 11 + 250
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c", "-std=c11", "-fsyntax-only", "-I", os.path.dirname(L.HEADER), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert L.ConvArgs is L.STRUCTS["sp_conv_args"] and dict(L.ConvArgs._fields_)["bnb"] is L.BnBwdArgs


def test_parser_refuses_what_it_does_not_understand():
    """a declaration outside the header's small grammar raises with the offending text: nothing is skipped or guessed"""
    import pytest
    ok = "typedef void* sp_stream_t;\ntypedef struct s { const float* p; int32_t a, b; } s;\nenum { X = 3 };\nint64_t sp_f(const s* a, double d, sp_stream_t st);\n"
    structs, sigs, consts = L.parse_header(ok)
    assert [n for n, _ in structs["s"]._fields_] == ["p", "a", "b"] and consts == {"X": 3}
    assert sigs == {"sp_f": ([L.vp, L.f64, L.vp], L.i64)}
    for bad, named in (("int sp_g(uint16_t n);", "uint16_t"),                                    # unknown type name
                       ("int sp_g(const sp_missing_args* a);", "sp_missing_args"),              # ... behind a pointer too
                       ("typedef struct t { int32_t a; float b;\nint sp_g(void);", "struct t"),  # unterminated struct
                       ("typedef struct t { int32_t a[4]; } t;", "a[4]"),                       # array member
                       ("typedef struct t { float *a, *b; } t;", "*b"),                         # mixed declarators
                       ("int sp_g(int32_t);", "int32_t"),                                       # unnamed parameter
                       ("enum { A, B };", "A"),                                                 # enum entry without a value
                       ("int sp_g(void (*cb)(int), int n);", "cb"),                             # function pointer
                       ("int sp_g(int n)", "sp_g")):                                            # no terminating semicolon
        with pytest.raises(ValueError, match=re.escape(named)):
            L.parse_header(ok + bad)


def test_every_declared_function_is_bound_with_its_parameter_count():
    src = re.sub(r"/\*.*?\*/", "", open(L.HEADER).read(), flags=re.S)
    decls = re.findall(r"\b(sp_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src)
    assert sorted(n for n, _ in decls) == _declared() == sorted(L.SIGS) and len(decls) >= 123
    for name, params in decls:
        want = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(L.SIGS[name][0]) == want, name
    lib = L.load()
    for name, (argtypes, restype) in L.SIGS.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    assert L.SIGS["sp_head_bwd_rows"] == ([L.i64], L.i64)
    assert L.SIGS["sp_head_row_floats"][1] is L.i32 and L.SIGS["sp_version"] == ([], L.i32)
    assert L.SIGS["sp_last_error"] == ([L.vp, ctypes.c_size_t], None)
    assert L.SIGS["sp_adam_step_flat"][0] == [L.vp] * 4 + [L.i64] + [L.f32] * 5 + [L.i32, L.f32, L.vp]
    assert L.SIGS["sp_sdm_plan"][0] == [L.i32, L.i32, L.i32, L.f64, L.i32, L.i32, L.vp, L.vp]
    assert (L.SP_BF16, L.SP_F32, L.SP_HL, L.SP_REDUCE_ROWS) == (0, 1, 2, 8)
    assert (L.ACT_NONE, L.ACT_LEAKY, L.ACT_ELU, L.ACT_SIGMOID) == (0, 1, 2, 3)


def test_version_and_error_text():
    lib = L.load()
    assert lib.sp_version() >= 100
    # argument validation happens before any GPU work: callable without a device
    rc = lib.sp_bn_stats(None, 0, 10, 8, None, None)
    assert rc == -1
    assert "sp_bn_stats" in L.last_error()


def test_zm_config_matches_the_planner():
    """sp_conv3d_zm_config (C side) and plan.ZM_CONFIGS (planner) describe the same kernels (no GPU needed: pure host code)"""
    import ctypes as C
    from stroke_prediction_amd.runtime import plan as P
    lib = L.load()
    for p in range(1, 8):
        for nt in range(1, 8):
            mt, ns, nw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
            rc = lib.sp_conv3d_zm_config(p, nt, C.byref(mt), C.byref(ns), C.byref(nw))
            if (p, nt) in P.ZM_CONFIGS:
                assert rc == 0 and (mt.value, ns.value, nw.value) == P.ZM_CONFIGS[(p, nt)], (p, nt)
            else:
                assert rc != 0, (p, nt)


def test_plane_serial_config_matches_the_planner():
    """sp_conv3d_zm_config_ps (plane-serial instances, round 5) and plan.ZM_CONFIGS_PS agree"""
    import ctypes as C
    from stroke_prediction_amd.runtime import plan as P
    lib = L.load()
    for nt in range(1, 5):
        for hl in (0, 1):
            mt, ns, nw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
            rc = lib.sp_conv3d_zm_config_ps(nt, hl, C.byref(mt), C.byref(ns), C.byref(nw))
            if (nt, bool(hl)) in P.ZM_CONFIGS_PS:
                assert rc == 0 and (mt.value, ns.value, nw.value) == P.ZM_CONFIGS_PS[(nt, bool(hl))], (nt, hl)
            else:
                assert rc != 0, (nt, hl)


def test_conv3d_plan_tables_match_the_planner():
    """sp_conv3d_plan / sp_conv3d_tables (the header-only caller's route to the z-marching kernel) build the same K tables
    as runtime/plan.py:zm_plan does for the Python host side, forward and data gradient (pure host code: no GPU)"""
    import ctypes as C
    import numpy as np
    from stroke_prediction_amd.runtime import plan as P
    lib = L.load()
    for cin, cout in ((16, 16), (16, 32), (32, 16), (32, 32), (48, 16), (16, 48)):
        for grad in (0, 1):
            dims = (20, 22, 40)
            d = L.Conv3dDesc(2, cin, cout, *dims, grad)
            pl = L.Conv3dPlan()
            op = (P.conv_dgrad_op(cin, cout, 3, 1, 0, dims, cout, cin, 0) if grad else
                  P.conv_fwd_op(cin, cout, 3, 1, 0, dims, cin, cout, 0))
            z = P.zm_plan(op)
            if z is not None:      # (the C planner keeps the classic tile: NW MT rows of 16 voxels)
                z = P.zm_plan(op, tile=(16, z["NW"] * z["MT"]))
            rc = lib.sp_conv3d_plan(C.byref(d), C.byref(pl))
            if z is None:
                assert rc != 0, (cin, cout, grad)
                continue
            assert rc == 0, L.last_error()
            assert (pl.P, pl.NT, pl.MT, pl.NW, pl.KS, pl.nsteps, pl.ITH) == (z["P"], z["NT"], z["MT"], z["NW"], z["KS"], z["nsteps"], z["ITH"])
            assert (pl.Do, pl.Ho, pl.Wo) == tuple(op.subs[0].out_dims) and (pl.o0, pl.o0H, pl.o0W) == tuple(op.subs[0].o0)
            assert (pl.Di, pl.Hi, pl.Wi) == tuple(op.in_dims)
            ktab = np.zeros(4 * pl.KS, np.int32); kmap = np.zeros(12 * pl.KS, np.int32)
            assert lib.sp_conv3d_tables(C.byref(d), C.byref(pl), ktab.ctypes.data, kmap.ctypes.data) == 0
            np.testing.assert_array_equal(ktab, z["ktab"])
            np.testing.assert_array_equal(kmap, z["kmap"])
            assert pl.workspace_bytes >= pl.off_wfrag + pl.nsteps * pl.NT * 1024 and pl.off_ktab >= 256
    # round 5: padded convolutions and their data gradients (the CAE's stride-1 layers) and stride-1 transposed convolutions
    for cin, cout, pad in ((16, 16, (1, 0, 0)), (32, 32, (1, 2, 2)), (16, 32, (1, 1, 1))):
        for kind in ("fwd", "grad", "convT"):
            dims = (9, 20, 22)
            d = L.Conv3dDesc(2, cin, cout, *dims, 1 if kind == "grad" else 0, *pad, 1 if kind == "convT" else 0)
            pl = L.Conv3dPlan()
            op = {"fwd": lambda: P.conv_fwd_op(cin, cout, 3, 1, pad, dims, cin, cout, 0),
                  "grad": lambda: P.conv_dgrad_op(cin, cout, 3, 1, pad, dims, cout, cin, 0),
                  "convT": lambda: P.convT_fwd_op(cin, cout, 3, 1, pad, dims, cin, cout, 0)}[kind]()
            z = P.zm_plan(op, tile="classic")
            assert z is not None and lib.sp_conv3d_plan(C.byref(d), C.byref(pl)) == 0, L.last_error()
            assert (pl.Di, pl.Hi, pl.Wi) == tuple(op.in_dims) and (pl.Do, pl.Ho, pl.Wo) == tuple(op.subs[0].out_dims), (kind, pad)
            assert (pl.o0, pl.o0H, pl.o0W) == tuple(op.subs[0].o0), (kind, pad, (pl.o0, pl.o0H, pl.o0W), op.subs[0].o0)
            ktab = np.zeros(4 * pl.KS, np.int32); kmap = np.zeros(12 * pl.KS, np.int32)
            assert lib.sp_conv3d_tables(C.byref(d), C.byref(pl), ktab.ctypes.data, kmap.ctypes.data) == 0
            np.testing.assert_array_equal(ktab, z["ktab"])
            np.testing.assert_array_equal(kmap, z["kmap"])
    # channel counts without a kernel, and malformed descriptors, are refused with a message
    bad = L.Conv3dDesc(1, 64, 64, 20, 20, 20, 0)
    assert lib.sp_conv3d_plan(C.byref(bad), C.byref(L.Conv3dPlan())) == -1 and "sp_conv3d_plan" in L.last_error()
    bad = L.Conv3dDesc(1, 8, 16, 20, 20, 20, 0)
    assert lib.sp_conv3d_plan(C.byref(bad), C.byref(L.Conv3dPlan())) == -1


def test_zm8_config_matches_the_planner():
    """sp_conv3d_zm8_config (fp8 kernel instances) and plan.ZM8_CONFIGS agree"""
    import ctypes as C
    from stroke_prediction_amd.runtime import plan as P
    lib = L.load()
    for p in range(1, 10):
        for nt in range(1, 6):
            mt, ns, nw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
            rc = lib.sp_conv3d_zm8_config(p, nt, C.byref(mt), C.byref(ns), C.byref(nw))
            if (p, nt) in P.ZM8_CONFIGS:
                assert rc == 0 and (mt.value, ns.value, nw.value) == P.ZM8_CONFIGS[(p, nt)], (p, nt)
            else:
                assert rc != 0, (p, nt)


def test_argument_validation_refuses_before_any_gpu_work():
    """every entry point checks its arguments on the host and returns SP_EINVAL with a message naming itself -- callable without
    a device, and what the sanitizer build (tools/build_asan.sh) walks through"""
    import ctypes as C
    lib = L.load()
    a = L.ConvArgs()
    for name in ("sp_conv3d_zm", "sp_conv3d_zm8"):
        assert getattr(lib, name)(C.byref(a), None, None) == -1 and name in L.last_error()
    assert lib.sp_conv3d_igemm(C.byref(a), None) == -1
    w = L.WgradArgs()
    assert lib.sp_conv3d_wgrad(C.byref(w), None) == -1
    f = L.ConvFcArgs()
    assert lib.sp_conv_fc(C.byref(f), None) == -1
    assert lib.sp_quantize_f8(None, 16, 0, None, 0, 10, 0, 1.0, None) == -1 and "sp_quantize_f8" in L.last_error()
    assert lib.sp_conv_prep_f8(None, 0, 0, 16, 16, None, 1, 1, None, None, None, 27, None, None, None, 1.0, None) == -1
    assert lib.sp_maxpool2_fwd_q8(None, None, 0, 1, 4, 4, 4, 16, None, None, 0, 0, 1.0, None) == -1
    assert lib.sp_bn_act_bwd_q8(None, None, None, 0, 10, 16, 1, 0.01, None, None, None, 0, 0, 1.0, None) == -1
    assert lib.sp_adam_step_flat(None, None, None, None, 10, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, None) == -1
    assert lib.sp_allreduce_flat(None, None, 10, None) == -1 and "sp_allreduce_flat" in L.last_error()


def test_pwout_argument_validation():
    """sp_pwout_fwd / _bwd / _finish refuse, with a message naming the entry point, a pitch other than 16, more than 16 channels, more than
    16 groups, coefficient rows closer than the three rows of pitch 16, and a group batch that does not divide the batch -- each with
    every other argument valid (non-null addresses that are never dereferenced: the checks run before any GPU work)"""
    import ctypes as C
    lib = L.load()
    buf = C.create_string_buffer(64)
    p = C.addressof(buf)

    def fwd(B=6, V=10, Cin=5, CP=16, coef=p, gstride=48, gb=2):
        return lib.sp_pwout_fwd(p, B, V, Cin, CP, coef, gstride, gb, p, p, p, None), "sp_pwout_fwd"

    def bwd(B=6, V=10, Cin=5, CP=16, gb=2, nrep=4):
        return lib.sp_pwout_bwd(p, p, p, B, V, Cin, CP, p, gb, nrep, p, p, None), "sp_pwout_bwd"

    def fin(nrep=4, G=3, Cin=5, coef=p, gstride=48):
        return lib.sp_pwout_finish(p, nrep, G, Cin, p, coef, gstride, p, 4, p, p, None), "sp_pwout_finish"

    SP_EINVAL = -1
    for fn, kw in ((fwd, dict(CP=8)), (bwd, dict(CP=8)), (fwd, dict(CP=32)), (bwd, dict(CP=32)),                                  # CP != 16
                   (fwd, dict(Cin=17)), (bwd, dict(Cin=17)), (fin, dict(Cin=17)),                                                 # Cin = 17
                   (fin, dict(G=17)),                                                                                             # G = 17
                   (fwd, dict(gstride=47)), (fin, dict(gstride=47)), (fwd, dict(gstride=16)), (fin, dict(gstride=0)),             # coef_gstride < 48
                   (fwd, dict(gb=4)), (bwd, dict(gb=4)), (fwd, dict(gb=-1)), (bwd, dict(gb=-1))):                                 # group_batch does not divide B = 6
        lib.sp_bn_stats(None, 0, 10, 8, None, None)      # (another entry point's message: the one read below is this call's own)
        rc, name = fn(**kw)
        assert rc == SP_EINVAL and name in L.last_error(), (name, kw, rc, L.last_error())


def test_rccl_unique_id_through_the_c_abi():
    """sp_comm_* resolve librccl at run time; creating a unique id needs no GPU"""
    import ctypes as C
    lib = L.load()
    if not lib.sp_comm_available():
        import pytest
        pytest.skip("no librccl in this process")
    a, b = C.create_string_buffer(128), C.create_string_buffer(128)
    assert lib.sp_comm_unique_id(a) == 0 and lib.sp_comm_unique_id(b) == 0
    assert a.raw != b.raw and any(a.raw)
    assert lib.sp_comm_init_rank(None, 1, a, 0) == -1


def test_sanitizer_build_of_the_host_code_passes_this_file():
    """SURVEY 5 / VERDICT r2 item 5c: the C ABI's host code under AddressSanitizer + UBSan (tools/build_asan.sh; the device
    code is untouched) runs this file clean.  The variant library is (re)built whenever it is missing or older than a source --
    and the test is never re-entered from the sanitizer run itself."""
    import subprocess
    import pytest
    if os.environ.get("SP_LIB_PATH", "").endswith("_asan.so"):
        pytest.skip("already inside the sanitizer run")
    so = os.path.join(ROOT, "stroke-prediction_amd", "lib", "variants", "libstroke_amd_asan.so")
    if not os.path.exists(os.path.join(ROOT, "tools", "build_asan.sh")):
        pytest.skip("CPU box only: the sanitizer scripts do not travel to the GPU pool (.gpurunignore)")
    # the variant must be as new as the sources: a missing or STALE one is rebuilt here (about two minutes, objects cached per
    # source under lib/variants/asan_obj), never skipped -- a skipped sanitizer run looks like a clean one
    srcs = [os.path.join(ROOT, "stroke-prediction_amd", "csrc", f) for f in os.listdir(os.path.join(ROOT, "stroke-prediction_amd", "csrc"))]
    srcs.append(os.path.join(ROOT, "include", "stroke_amd.h"))
    if os.environ.get("SP_RUN_ASAN") == "1" or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([os.path.join(ROOT, "tools", "build_asan.sh")], check=True, timeout=1500)
    assert os.path.exists(so) and all(os.path.getmtime(s) <= os.path.getmtime(so) for s in srcs), "tools/build_asan.sh left a stale variant"
    # with a GPU present, RCCL brings the ROCm runtime up inside the instrumented process, which aborts it: there the RCCL id test
    # (host plumbing, run un-instrumented in this file as well) stays out of the sanitizer run
    import torch
    deselect = ["-k", "not test_rccl_unique_id_through_the_c_abi"] if torch.cuda.is_available() else []
    r = subprocess.run([os.path.join(ROOT, "tools", "run_asan_tests.sh")] + deselect, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "passed" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
