"""CPU: every ctypes signature of the bindings comes from include/vido_c.h (vido_slam_amd.host.parse_header / load_library).  The hand-written tables the parser replaced
are kept here as literal expected values, and an AST walk over the package checks the call sites the declared signatures now convert for."""
import ast
import ctypes as C
import os

import numpy as np
import pytest

from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vido-slam_amd")

# (restype, argtypes) as the bindings declared them by hand before the header was parsed (host.load_library, system._bind, host.rccl_direct_init and the two restype lines
# of nets/ops.py): p pointer, s char*, i int, u unsigned, z size_t, f float, d double, q long long; "" = the default int return
HAND = {
    "vido_last_error": ("s", "p"),
    "vido_create": ("", "pp"),
    "vido_destroy": ("", "p"),
    "vido_stream": ("p", "p"),
    "vido_synchronize": ("", "p"),
    "vido_orb_extract": ("", "ppiiipipp"),
    "vido_orb_extract_batch": ("", "ppiiziiipipp"),
    "vido_orb_extract_color": ("", "ppiiiiziiippipp"),
    "vido_orb_level_size": ("", "pipp"),
    "vido_orb_read_level": ("", "piiip"),
    "vido_orb_read_candidates": ("", "piipi"),
    "vido_orb_last_timing": ("", "pp"),
    "vido_orb_geometry": ("", "pp"),
    "vido_hamming_match": ("", "ppipippi"),
    "vido_hamming_match_window": ("", "ppppipppifiiiiipppppi"),
    "vido_orb_describe_points": ("", "pipippppi"),
    "vido_orb_patch_points": ("", "pipiipiipppi"),
    "vido_orb_patch_search": ("", "pipiipiiiiipppppi"),
    "vido_orb_patch_refine": ("", "pipiipiiipppppi"),
    "vido_dis_flow": ("", "pppiiiiiiiiipppi"),
    "vido_flow_consistency": ("", "pppiiiipppi"),
    "vido_dis_flow_pair": ("", "pppiiiiiiiiiiipppppi"),
    "vido_device_name": ("", "psi"),
    "vido_mask_propagate": ("", "ppppiipp"),
    "vido_frame_propagate_mask": ("", "piip"),
    "vido_mask_associate": ("", "pppiipiipppp"),
    "vido_mask_components": ("", "ppiiiiiipppp"),
    "vido_frame_split_mask": ("", "piiiiip"),
    "vido_rccl_unique_id": ("", "p"),
    "vido_rccl_init": ("", "ppii"),
    "vido_system_create": ("", "sp"),
    "vido_system_destroy": ("", "p"),
    "vido_system_last_error": ("s", "p"),
    "vido_system_track_rgbd": ("", "ppiiipppdip"),
    "vido_system_track_rgbd_device": ("", "ppiiippppdip"),
    "vido_system_get_stats": ("", "pp"),
    "vido_system_save_results": ("", "ps"),
    "vido_system_context": ("p", "p"),
    "vido_system_set_depth_noise_seed": ("", "pu"),
    "vido_system_set_zero_copy_maps": ("", "pi"),
    "vido_system_prefetch_image_device": ("", "ppiiip"),
    "vido_system_get_verify_stats": ("", "ppp"),
    "vido_system_mask_split_stats": ("", "pp"),
    "vido_system_get_verify_points": ("", "pppppppip"),
    "vido_system_get_recover_stats": ("", "ppp"),
    "vido_system_get_recover_points": ("", "pppppppipppppip"),
    "vido_system_get_object_verify_stats": ("", "pppp"),
    "vido_system_get_object_verify_points": ("", "ppppppip"),
    "vido_system_get_object_recover_stats": ("", "ppp"),
    "vido_system_get_object_recover_points": ("", "pppppppip"),
    "vido_system_get_object_refine_stats": ("", "ppp"),
    "vido_system_get_object_refine_points": ("", "ppppip"),
    "vido_conv_direct_packed_floats": ("q", None),       # (only the return type was declared)
    "vido_wino3x3_packed_floats_form": ("q", None),
}
CODE = {"p": C.c_void_p, "s": C.c_char_p, "i": C.c_int, "u": C.c_uint, "z": C.c_size_t, "f": C.c_float, "d": C.c_double, "q": C.c_longlong, "": C.c_int}
FLOATS = (C.c_float, C.c_double)
# the nine returns of the header that are neither int nor void
RETURNS = {"vido_last_error": C.c_char_p, "vido_system_last_error": C.c_char_p, "vido_stream": C.c_void_p, "vido_system_context": C.c_void_p}


def header_text():
    with open(os.path.join(ROOT, "include", "vido_c.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def sigs():
    from vido_slam_amd.host import parse_header
    return parse_header(header_text())


def same_class(a, b):
    """two ctypes types pass the same way: same size, both floating point or neither"""
    return C.sizeof(a) == C.sizeof(b) and (a in FLOATS) == (b in FLOATS)


def test_parser_finds_every_declared_symbol(sigs):
    assert set(sigs) == set(declared_symbols())


def test_parser_agrees_with_the_hand_written_tables(sigs):
    for name, (res, args) in HAND.items():
        restype, argtypes = sigs[name]
        if res or restype is not None:                               # (a void function was called with the default return type, its value unused)
            assert restype is not None and same_class(restype, CODE[res]), (name, restype)
        if res in ("s", "p"):
            assert restype is CODE[res], (name, restype)            # a char* return is decoded, a pointer return is not truncated: the type itself matters
        if args is not None:
            assert len(argtypes) == len(args), (name, len(argtypes), len(args))
            for k, (got, want) in enumerate(zip(argtypes, args)):
                assert same_class(got, CODE[want]), (name, k, got, want)
                if want == "s":
                    assert got is C.c_char_p, (name, k, got)


def test_mapping_of_every_kind(sigs):
    from vido_slam_amd.host import parse_header
    s = parse_header("""
        /* a comment with vido_not_a_function( in it */
        long long vido_a(const vido_ctx* ctx, float w[4], unsigned seed, uint32_t m, int32_t k, size_t n, long long hw, int64_t c, uint64_t s, double d, float f,
                         const char* path, char* buf, vido_allreduce_fn fn, void* user, int);
        void vido_b(void);
        vido_ctx* vido_c(void);
        const char* vido_d(const vido_ctx*);
        float vido_e(int a);   // trailing comment
        int64_t vido_f();
    """)
    assert s["vido_a"] == (C.c_longlong, [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint32, C.c_int32, C.c_size_t, C.c_longlong, C.c_int64, C.c_uint64, C.c_double, C.c_float,
                                          C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int])
    assert s["vido_b"] == (None, []) and s["vido_c"] == (C.c_void_p, []) and s["vido_d"] == (C.c_char_p, [C.c_void_p])
    assert s["vido_e"] == (C.c_float, [C.c_int]) and s["vido_f"] == (C.c_int64, [])
    assert set(s) == {"vido_a", "vido_b", "vido_c", "vido_d", "vido_e", "vido_f"}
    # undeclared-before functions of each risky kind, from the real header
    assert sigs["vido_conv1x1_skinny"][1][-2] is C.c_longlong and sigs["vido_bias_act"][1][-1] is C.c_float and sigs["vido_gconv3x3_packed_size"][0] is C.c_int64


@pytest.mark.parametrize("text, name", [("int vido_ok(int a);\nint vido_bad_type(vido_ctx* ctx, short n);", "vido_bad_type"),
                                        ("short vido_bad_return(int a);", "vido_bad_return"),
                                        ("int vido_bad_shape(int (*cb)(int), int n);", "vido_bad_shape"),
                                        ("int vido_unfinished(int a, int b)", "vido_unfinished"),
                                        ("int vido_twice(int a);\nint vido_twice(int a, int b);", "vido_twice")])
def test_parser_raises_with_the_functions_name(text, name):
    from vido_slam_amd.host import parse_header
    with pytest.raises(ValueError, match=name):
        parse_header(text)


def test_library_is_bound_from_the_header(sigs, monkeypatch):
    from vido_slam_amd import host
    monkeypatch.setattr(host, "_lib", None)                  # a handle of its own: other tests re-declare a debug hook on the shared one
    lib = host.load_library()
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    odd = {n: r for n, (r, _) in sigs.items() if r not in (C.c_int, None)}
    assert len(odd) == 9 and all(getattr(lib, n).restype is r and r is not C.c_int for n, r in odd.items()), odd
    for n, r in RETURNS.items():
        assert odd[n] is r
    assert sorted(C.sizeof(r) for r in odd.values()) == [4] + [8] * 8             # one float; everything else is 64 bits wide and would be cut to 32 undeclared
    assert lib.vido_conv1x1_skinny.argtypes[-2] is C.c_longlong and lib.vido_bias_act.argtypes[-1] is C.c_float and lib.vido_gconv3x3_packed_size.restype is C.c_int64


def test_missing_header_fails_like_a_missing_library(monkeypatch):
    from vido_slam_amd import host
    monkeypatch.setattr(host, "_lib", None)
    monkeypatch.setattr(host, "HEADER_PATH", os.path.join(ROOT, "include", "no_such_header.h"))
    with pytest.raises(host.VidoError, match="no_such_header.h not found") as e:
        host.load_library()
    assert e.value.code == -2


def test_from_param_accepts_what_the_call_sites_pass():
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)
    a = np.zeros(4, np.float32)
    for v in (None, 0, (1 << 47) + 8, C.byref(C.c_int()), (C.c_float * 4)(1, 2, 3, 4), (C.c_void_p * 2)(), a.ctypes.data_as(C.c_void_p), a.ctypes.data, C.c_void_p(5),
              cb(lambda *_: 0), C.cast(None, cb), C.byref(C.c_void_p())):
        C.c_void_p.from_param(v)
    C.c_char_p.from_param(C.create_string_buffer(16)); C.c_char_p.from_param(b"x"); C.c_char_p.from_param(None)
    assert C.c_float.from_param(3) is not None and C.c_double.from_param(2) is not None and C.c_longlong.from_param(1 << 40) is not None
    C.c_float.from_param(np.float32(0.25)); C.c_int.from_param(True); C.c_size_t.from_param(0); C.c_uint64.from_param(1)
    with pytest.raises((TypeError, C.ArgumentError)):
        C.c_void_p.from_param(1.5)
    with pytest.raises((TypeError, C.ArgumentError)):
        C.c_int.from_param(1.5)


# ---- the call sites --------------------------------------------------------------------------------------------------------------------------------------------------
WRAPPERS = ("c_void_p", "c_float", "c_longlong", "c_int64")


def header_calls(tree, names):
    """(name, argument nodes, lineno) of every call of a header function in `tree`: `<expr>.vido_x(args)`, and `<expr>._call(<expr>.vido_x, args)` — HipOps._call, which
    passes the context handle first.  Calls with *args are left out."""
    for node in ast.walk(tree):
        if not isinstance(node, ast.Call) or not isinstance(node.func, ast.Attribute):
            continue
        if node.func.attr in names:
            name, args, extra = node.func.attr, node.args, 0
        elif node.func.attr == "_call" and node.args and isinstance(node.args[0], ast.Attribute) and node.args[0].attr in names:
            name, args, extra = node.args[0].attr, node.args[1:], 1
        else:
            continue
        if any(isinstance(a, ast.Starred) for a in args) or node.keywords:
            continue
        yield name, args, extra, node.lineno


def package_files():
    for dp, _, fns in os.walk(PKG):
        for fn in sorted(fns):
            if fn.endswith(".py"):
                yield os.path.join(dp, fn)


def test_call_sites_pass_the_headers_argument_count(sigs):
    bad, seen = [], 0
    for path in package_files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for name, args, extra, line in header_calls(tree, sigs):
            seen += 1
            if len(args) + extra != len(sigs[name][1]):
                bad.append("%s:%d %s passes %d arguments, the header declares %d" % (os.path.relpath(path, ROOT), line, name, len(args) + extra, len(sigs[name][1])))
    assert not bad, "\n".join(bad)
    assert seen >= 150, seen                   # the walk sees the package's calls (176 when this was written), HipOps._call's included


def test_call_sites_carry_no_ctypes_casts(sigs):
    bad = []
    for path in package_files():
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for name, args, _, line in header_calls(tree, sigs):
            for a in args:
                for n in ast.walk(a):
                    if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr in WRAPPERS and isinstance(n.func.value, ast.Name) and n.func.value.id in ("C", "ctypes"):
                        bad.append("%s:%d %s: %s.%s(...)" % (os.path.relpath(path, ROOT), line, name, n.func.value.id, n.func.attr))
    assert not bad, "\n".join(bad)


# ---- GPU: plain Python scalars and pointers through functions that had no declared signature --------------------------------------------------------------------------
@pytest.mark.gpu
def test_plain_scalars_reach_the_kernels():
    import torch
    import vido_slam_amd as V
    from vido_slam_amd.nets.ops import HipOps
    ops = HipOps(V.Context())
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 8, 5, 7), generator=g).cuda(); b = torch.randn((8,), generator=g).cuda()
    want = torch.nn.functional.leaky_relu(x + b[None, :, None, None], 0.25)
    got = ops.bias_act_(x.clone(), b, 0.25)
    assert torch.equal(got, want)
    # the LevelMapper expression of nets/maskrcnn.py::_Pooler.forward, which roi_levels replaces; sides from 1 to ~1100 px cover every level of 2 .. 5
    xy = torch.rand((16, 2), generator=g) * 300; wh = torch.exp(torch.rand((16, 2), generator=g) * 7)
    boxes = torch.cat([xy, xy + wh], 1).cuda()
    k_min, k_max = 2.0, 5.0
    area = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    want = torch.floor(4 + torch.log2(torch.sqrt(area) / 224 + 1e-6)).clamp(min=k_min, max=k_max).to(torch.int64) - int(k_min)
    got = ops.roi_levels(boxes, k_min, k_max)
    assert got.dtype == torch.int32 and torch.equal(got.to(torch.int64), want)
