"""CPU-side checks: the C-ABI library builds, loads and exports every symbol include/te_hip.h declares;
the product path refuses to run without a GPU (no silent fallback); host-side shape logic and the
state_dict schema match the reference."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope='module')
def libpath():
    from transeditor_amd import build
    return build.build(verbose=False)


def test_library_exports_every_declared_symbol(libpath):
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    declared = sorted(set(re.findall(r'\b(te_[a-z0-9_]+)\s*\(', header)))
    assert len(declared) >= 14
    lib = ctypes.CDLL(libpath)
    missing = [n for n in declared if not hasattr(lib, n)]
    assert not missing, missing
    lib.te_arch.restype = ctypes.c_char_p
    assert lib.te_arch() == b'gfx950'
    assert lib.te_version() == 3


def test_binding_table_matches_header(libpath):
    from transeditor_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    declared = set(re.findall(r'\b(te_[a-z0-9_]+)\s*\(', header))
    assert declared == set(_lib.EXPORTS)
    assert _lib.lib().te_version() == 3


def _declared_prototypes():
    """{name: parameter list text} by a regex of this file's own (not the product's parser), on the header without comments"""
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    header = re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    return dict(re.findall(r'\b(te_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', header))


def test_bindings_pinned_by_hand():
    """the prototypes lib() binds are READ from include/te_hip.h; a dozen of them written out here by hand, one for every type of the
    vocabulary and for the awkward shapes (no arguments, char* results, runs of doubles, out-parameters, pointer arrays, 24 arguments)"""
    from transeditor_amd import _abi
    P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    table = _abi.parse(open(os.path.join(ROOT, 'include', 'te_hip.h')).read())
    want = {
        'te_version': (I, []),
        'te_last_error_string': (ctypes.c_char_p, []),
        'te_arch': (ctypes.c_char_p, []),
        'te_bias_act_bwd_ws_floats': (L, [L, L, L]),
        'te_mt_adam_f32': (I, [P, P, I, I, I, D, D, D, D, I, P]),
        'te_svm_smo_f64': (I, [P, P, P, P, P, I, D, D, L, P]),
        'te_upfirdn2d_f32': (I, [P, P, P, L, I, I, I, I, I, I, I, I, I, I, I, I, I, P, L, I, F, F, P]),
        'te_small_gemm_batched_f32': (I, [P, P, P, P, I, L, L, L, L, P, P, I, I, I, L, L, L, L, L, L, F, F, I, P]),
        'te_wgrad_group_plan': (I, [I, I, I, I, I, I, P, P]),
        'te_conv_form': (I, [I, I, I, I, I, I, I, I, I, P]),
        'te_small_gemm_form': (I, [I, I, I, I, L, L, L, L, L, L, P, I, I, I, P]),
        'te_wgrad_form': (I, [I, I, I, I, I, I, I, I, I, I, P]),
        'te_fir_form': (I, [I, L, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
        'te_lpips_allpairs_dist_f32': (I, [P, P, P, P, I, I, P]),
        'te_conv2d_prelu_f32': (I, [P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, P]),
        'te_fid_moments_f64': (I, [P, P, P, P, L, I, I, P]),
    }
    assert len(want['te_upfirdn2d_f32'][1]) == 23 and len(want['te_small_gemm_batched_f32'][1]) == 24
    for name, (res, args) in want.items():
        got_res, got_args = table[name]
        assert got_res is res, name
        assert len(got_args) == len(args) and all(a is b for a, b in zip(got_args, args)), (name, got_args)


def test_every_binding_has_the_declared_number_of_arguments(libpath):
    from transeditor_amd import _lib
    declared = _declared_prototypes()
    assert tuple(declared) == _lib.EXPORTS and len(declared) >= 150         # header order
    L = _lib.lib()
    for name, params in declared.items():
        n = 0 if params.strip() == 'void' else params.count(',') + 1       # (no nested parentheses: every comma is top-level)
        assert len(getattr(L, name).argtypes) == n, name


def test_header_parser_on_synthetic_headers():
    from transeditor_amd import _abi
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    text = """
    #ifndef X
    #define TE_ABI_VERSION 7
    /* int te_in_block_comment(int a);
       te_bias_act_bwd_ws_floats(outer, C, inner) floats */
    // int te_in_line_comment(int a);
    typedef void* te_stream_t;
    enum { TE_A = 0, TE_B = 1 };
    int64_t
    te_four_lines(const float* const* p,     /* a comment between parameters */
                  int64_t const n, float w[3],
                  te_stream_t stream);
    const char* te_name(void);
    double te_unnamed(int, const double*, float, int64_t);
    int te_empty();
    #endif
    """
    table = _abi.parse(text)
    assert list(table) == ['te_four_lines', 'te_name', 'te_unnamed', 'te_empty']
    assert table['te_four_lines'] == (L, [P, L, P, P])
    assert table['te_name'] == (ctypes.c_char_p, [])
    assert table['te_unnamed'] == (ctypes.c_double, [I, P, F, L])
    assert table['te_empty'] == (I, [])
    assert _abi.abi_version(text) == 7
    for bad in ('int te_bad(size_t n);', 'int te_bad(int a, struct foo x);', 'int te_bad(unsigned int n);', 'void te_bad(int n);',
                'float* te_bad(int n);', 'int te_bad(int (*cb)(int));'):
        with pytest.raises(RuntimeError, match='te_bad'):
            _abi.parse(bad)
    with pytest.raises(RuntimeError, match='TE_ABI_VERSION'):
        _abi.abi_version('int te_version(void);')


def test_missing_header_and_stale_library_are_refused(libpath, monkeypatch, tmp_path):
    """lib() refuses to bind without the header, and a library whose te_version() is not the header's TE_ABI_VERSION"""
    from transeditor_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'te_hip.h')).read()
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, 'include', 'te_hip.h'))
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, '_protos', None)
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'te_hip.h'))
    with pytest.raises(RuntimeError, match='te_hip.h is missing'):
        _lib.lib()
    assert '#define TE_ABI_VERSION 3' in header
    monkeypatch.setattr(_lib, '_header_text', lambda: header.replace('#define TE_ABI_VERSION 3', '#define TE_ABI_VERSION 4'))
    with pytest.raises(RuntimeError, match='ABI version 3 but include/te_hip.h declares 4'):
        _lib.lib()
    assert _lib._lib is None
    monkeypatch.undo()
    assert _lib.lib().te_version() == 3


def test_launch_sites_name_their_entry_point_once():
    """every launch goes through _launch(name, ...): no `_check(lib().te_x(..., _stream()), 'te_x')` with its second copy of the name
    is left; what still calls _check is _launch itself and the host-only plan query"""
    src = open(os.path.join(ROOT, 'transeditor_amd', '_lib.py')).read()
    calls = [m.start() for m in re.finditer(r'\b_check\(', src)]
    stmts = [src[i:src.index('\n\n', i)] for i in calls]
    assert not [s for s in stmts if '_check(lib().' in s and '_stream()' in s]
    assert len([s for s in stmts if not s.startswith('_check(rc, what)')]) == 2
    assert src.count("_launch('te_") >= 75
    for f in ('frozen_net.py',):
        assert '_check(' not in open(os.path.join(ROOT, 'transeditor_amd', f)).read()


def test_argument_validation_returns_error_codes(libpath):
    """No compute without a GPU: only the host-side validation paths are exercised."""
    from transeditor_amd import _lib
    L = _lib.lib()
    assert L.te_bias_act_f32(None, None, None, None, 3, 0, 0.2, 1.0, 16, 1, 1, None) == -1
    assert b'NULL' in L.te_last_error_string()
    assert L.te_conv_packed_numel(0, 5, 6, 3) == 9 * 16 * 128
    assert L.te_conv_packed_numel(1, 512, 256, 3) == 9 * 512 * 256
    assert L.te_wgrad_slab_count(0, 16, 128, 128, 256, 256) >= 1
    assert L.te_wgrad_slab_count(0, 0, 128, 128, 256, 256) < 0
    # host-side plans of the Winograd forms (pure functions of the shape)
    assert L.te_conv_wino_supported(16, 128, 128, 256, 256) == 1 and L.te_conv_wino_supported(16, 128, 128, 16, 16) == 0
    assert L.te_conv_wino_supported(16, 3, 128, 256, 256) == 0 and L.te_conv_wino_supported(4, 32, 32, 1024, 1024) == 1
    assert L.te_conv_packed_numel(_lib.PACK_WFWD, 128, 256, 3) == 12 * 128 * 256
    assert L.te_wgrad_pair_form(0, 128, 128, 256, 256) == 1 and L.te_wgrad_pair_form(0, 64, 64, 512, 512) == 0
    assert L.te_conv_wino6_supported(16, 128, 128, 256, 256) == 1 and L.te_conv_wino6_supported(4, 64, 64, 512, 512) == 1
    assert L.te_conv_wino6_supported(4, 32, 32, 1024, 1024) == 0 and L.te_conv_wino6_supported(16, 512, 512, 8, 8) == 0        # M % 64, W % 32 ...
    assert L.te_conv_wino6_supported(16, 512, 512, 16, 16) == 1 and L.te_conv_wino6_supported(15, 512, 512, 16, 16) == 0    # ... or W == 16, even batch (round 6)
    assert L.te_conv_wino6_supported(16, 48, 64, 32, 32) == 0                                                                    # K % 32
    assert L.te_conv_packed_numel(_lib.PACK_W6FWD, 128, 256, 3) == 18 * 128 * 256 == L.te_conv_packed_numel(_lib.PACK_W6DGRAD, 128, 256, 3)
    assert L.te_wgrad_pair_form(1, 128, 128, 64, 64) == 0 and L.te_wgrad_pair_form(0, 128, 128, 1, 1) == 0


def test_product_path_fails_loudly_on_cpu(libpath):
    from transeditor_amd.op import fused_leaky_relu, upfirdn2d
    from transeditor_amd.op.modconv import modconv
    with pytest.raises(RuntimeError, match='GPU'):
        fused_leaky_relu(torch.randn(2, 4), torch.zeros(4))
    with pytest.raises(RuntimeError, match='GPU'):
        upfirdn2d(torch.randn(1, 1, 8, 8), torch.ones(4, 4) / 16, pad=(1, 1))
    with pytest.raises(RuntimeError, match='GPU'):
        modconv(torch.randn(1, 8, 4, 4), torch.randn(8, 8, 3, 3))
    # the dense / normalisation ops of the mapping and attention stack have no CPU route either
    from transeditor_amd.op.layernorm import pixel_norm, sample_layer_norm
    from transeditor_amd.op.linear import linear_fused
    from transeditor_amd.op.style import demod
    from transeditor_amd.op.token_mlp import token_mlp
    with pytest.raises(RuntimeError, match='GPU'):
        linear_fused(torch.randn(4, 8), torch.randn(6, 8), torch.zeros(6))
    with pytest.raises(RuntimeError, match='GPU'):
        sample_layer_norm(torch.randn(2, 4, 8))
    with pytest.raises(RuntimeError, match='GPU'):
        pixel_norm(torch.randn(2, 8, 4), 1)
    with pytest.raises(RuntimeError, match='GPU'):
        token_mlp(torch.randn(2, 8, 4), [torch.randn(8, 8)] * 4, [torch.zeros(8)] * 4, 1.0, 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        demod(torch.randn(8, 8, 3, 3), torch.randn(2, 8), 1.0)


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'transeditor_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, re.M), os.path.join(dirpath, f)
                assert '/root/reference' not in src, os.path.join(dirpath, f)


@pytest.mark.parametrize('tag,ctor', [('g64', ('G', 64, 10)), ('g256', ('G', 256, 14)), ('g1024', ('G', 1024, 18)),
                                      ('d64', ('D', 64, 0)), ('d256', ('D', 256, 0))])
def test_state_dict_schema_matches_reference(golden, tag, ctor):
    from transeditor_amd.model_spatial_query import Discriminator, Generator
    g = golden('state_dict_schema')
    kind, size, token = ctor
    m = Generator(size, 512, 512, token, n_trans=8, pixel_norm_op_dim=1) if kind == 'G' else Discriminator(size)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[tag + '.keys']]
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[tag + '.shapes']]
    assert sum(p.numel() for p in m.parameters()) == int(g[tag + '.nparams'])
    assert [n for n, _ in m.named_parameters()] == [str(k) for k in g[tag + '.param_names']]


def test_upfirdn2d_geometry_formulas():
    """out size and adjoint padding (utils/op/upfirdn2d.py:101-112 in the reference): integer, exact."""
    from transeditor_amd.op.upfirdn2d import _geometry
    # blur pad (1,1) on 2H+1 -> 2H ; adjoint pads (2,2)
    assert _geometry((9, 9), (4, 4), (1, 1), (1, 1), (1, 1, 1, 1)) == ((8, 8), (2, 2, 2, 2))
    # D blur pad (2,2) -> adjoint (1,1)
    assert _geometry((8, 8), (4, 4), (1, 1), (1, 1), (2, 2, 2, 2)) == ((9, 9), (1, 1, 1, 1))
    # skip upsample x2 pad (2,1) -> adjoint (1,1)
    assert _geometry((5, 7), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1)) == ((10, 14), (1, 1, 1, 1))


def test_synth_is_deterministic_and_normal():
    from transeditor_amd import synth
    a = synth.normal((4096,), 'unit.test', 3)
    b = synth.normal((4096,), 'unit.test', 3)
    assert torch.equal(a, b)
    assert abs(float(a.mean())) < 0.06 and abs(float(a.std()) - 1) < 0.05
    assert not torch.equal(a, synth.normal((4096,), 'unit.test', 4))
    # pinned values: the GPU box must regenerate exactly these
    assert np.allclose(a[:3].numpy(), synth.normal((3,), 'unit.test', 3).numpy())


def test_generator_ctor_surface():
    import inspect
    from transeditor_amd.model_spatial_query import Generator, ModulatedConv2d
    sig = inspect.signature(Generator.__init__)
    assert list(sig.parameters)[1:] == ['size', 'style_dim', 'param_dim', 'token_dim', 'channel_multiplier', 'blur_kernel',
                                        'lr_mlp', 'layer_noise_injection', 'use_spatial_mapping', 'num_region', 'n_trans',
                                        'pixel_norm_op_dim', 'no_trans']
    assert sig.parameters['n_trans'].default == 4 and sig.parameters['pixel_norm_op_dim'].default == 2
    fsig = inspect.signature(Generator.forward)
    assert list(fsig.parameters)[1:] == ['style', 'op_param', 'return_latents', 'input_is_latent', 'noise',
                                         'randomize_noise', 'return_style', 'return_p_latent', 'return_only_style',
                                         'return_only_style_latent', 'return_only_mapped_p', 'return_only_mapped_z',
                                         'use_spatial_mapping', 'use_style_mapping', 'trans_interact',
                                         'return_mapped_codes']
    g = Generator(32, 512, 512, 8, n_trans=2)
    assert g.n_latent == 8 and g.num_layers == 7 and len(g.convs) == 6 and len(g.to_rgbs) == 3
    assert list(inspect.signature(ModulatedConv2d.__init__).parameters)[1:9] == [
        'in_channel', 'out_channel', 'kernel_size', 'style_dim', 'demodulate', 'upsample', 'downsample', 'blur_kernel']


def test_train_step_losses_match_oracle_on_cpu():
    """Loss formulas of the train-step harness (pure torch) against the oracle's restatement."""
    from oracle import te_oracle as O
    from transeditor_amd import synth, train_step as T
    rp, fp = synth.normal((6, 1), 'l.r'), synth.normal((6, 1), 'l.f')
    assert torch.allclose(T.d_logistic_loss(rp, fp), O.d_logistic_loss(rp, fp))
    assert torch.allclose(T.g_nonsaturating_loss(fp), O.g_nonsaturating_loss(fp))
    lat = synth.normal((2, 4, 8), 'l.lat').requires_grad_(True)
    A = synth.normal((8, 3 * 4 * 4), 'l.A')
    img = torch.tanh(lat.sum(1) @ A).reshape(2, 3, 4, 4)
    noise = synth.normal((2, 3, 4, 4), 'l.n')
    a = T.g_path_regularize(img, lat, 0.0, noise)
    b = O.g_path_regularize(img, lat, 0.0, noise / 4.0)
    assert torch.allclose(a[0], b[0]) and torch.allclose(a[2], b[2])
    m1, m2 = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    with pytest.raises(RuntimeError, match='no CPU path'):        # the EMA is a HIP kernel (tests/test_gpu_optim.py)
        T.accumulate(m1, m2, 0.9)
    args = T.default_args(size=64)
    assert args.token == 10 and args.d_reg_every == 16 and args.g_reg_every == 4


def test_modconv_host_argument_logic():
    """activation-gain codes and the demodulation argument contract are decided on the host, before any launch"""
    from transeditor_amd.op import modconv as M
    assert M._act_code(False) == 0 and M._act_code(True) == 3 and M._act_code(2 ** 0.5) == 3 and M._act_code(1.0) == 4
    assert M._act_code(2 ** 0.5 * (1 / 2 ** 0.5)) == 4                       # ResBlock: sqrt(2) * 1/sqrt(2)
    with pytest.raises(RuntimeError, match='gain'):
        M._act_code(0.5)
    x, w = torch.randn(1, 8, 4, 4), torch.randn(8, 8, 3, 3)
    with pytest.raises(RuntimeError, match='demod_eps'):
        M.modconv(x, w, isc=torch.ones(1, 8), osc=torch.ones(1, 8), demod_eps=1e-8)
    with pytest.raises(RuntimeError, match='demod_eps'):
        M.modconv(x, w, demod_eps=1e-8)                                       # demodulation without a style scale
    dgrad_pack = lambda op: M._PACK[M._ROUTES[M._ADJOINT[op]][0]][True]      # (layout the fp32 data gradient of `op` reads)
    assert dgrad_pack('up') == dgrad_pack('down') != dgrad_pack('3x3')
    from transeditor_amd.op import weight_cache
    with M.second_order(), M.no_weight_grads():
        assert M._STATE.second_order is True and M.weights_skipped() is True
    assert M._STATE.second_order is False and M.weights_skipped() is False
    # forward-side hints and the frozen-weight cache are thread-local (nn.DataParallel worker threads, a sampler next to a
    # training loop); the skip flag travels on a token the nodes keep, because backward runs on the autograd engine's thread
    import threading
    seen = {}

    def other():
        seen['so'] = M._STATE.second_order
        seen['frozen'] = weight_cache._CACHES.frozen_on
        seen['graph_is_default'] = M.current_graph() is M._DEFAULT_GRAPH
    with M.second_order() as tok, weight_cache.frozen_weights({}):
        assert weight_cache._CACHES.frozen_on is True
        assert M.current_graph() is tok and tok is not M._DEFAULT_GRAPH
        t = threading.Thread(target=other)
        t.start()
        t.join()
    assert seen == {'so': False, 'frozen': False, 'graph_is_default': True}
    with M.no_weight_grads():                       # flips the token of the forward that just ended (and the default one)
        assert tok.skip_w and M._DEFAULT_GRAPH.skip_w
    assert not tok.skip_w and not M._DEFAULT_GRAPH.skip_w


def test_upfirdn2d_geometry_matches_reference_formulas():
    """output size and adjoint pads (utils/op/upfirdn2d.py:101-112) for the five configurations the model uses"""
    from transeditor_amd.op.upfirdn2d import _geometry
    # blur pad (1,1) on 257 -> 256, its adjoint pads (1,3): 256 -> 257
    (oh, ow), g_pad = _geometry((257, 257), (4, 4), (1, 1), (1, 1), (1, 1, 1, 1))
    assert (oh, ow) == (256, 256) and g_pad == (2, 2, 2, 2)
    (oh, ow), _ = _geometry((256, 256), (4, 4), (1, 1), (1, 1), g_pad)
    assert (oh, ow) == (257, 257)
    # ToRGB skip upsample: up 2, pad (2,1): 128 -> 256; adjoint is down 2
    (oh, ow), g_pad = _geometry((128, 128), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1))
    assert (oh, ow) == (256, 256) and g_pad == (1, 1, 1, 1)
    # discriminator blur pad (2,2) before the stride-2 3x3: 256 -> 257; skip branch blur (1,1) with down 2: 256 -> 128
    assert _geometry((256, 256), (4, 4), (1, 1), (1, 1), (2, 2, 2, 2))[0] == (257, 257)
    assert _geometry((256, 256), (4, 4), (1, 1), (2, 2), (1, 1, 1, 1))[0] == (128, 128)


def test_tools_and_entry_points_compile():
    """the GPU-side diagnostics under tools/ (run only on the GPU box) at least parse, so a visit is never lost to a typo"""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, 'tools', '*.py')) + [os.path.join(root, 'bench.py'), os.path.join(root, '__graft_entry__.py')]
    assert len(files) > 10
    for f in files:
        compile(open(f).read(), f, 'exec')


_RANGED_BEFORE = [          # the hand-kept list _install_roctx had: the floor of what carries a range
    'bias_act', 'bias_act_bwd', 'upfirdn2d_raw', 'blur_actgrad', 'blur_gradact', 'conv_pack', 'conv_pack2', 'conv_pack_multi', 'conv',
    'wgrad_slabs', 'wgrad_reduce', 'rgb_fwd', 'rgb_dgrad', 'rgb_expand', 'rgb_wgrad_slabs', 'small_gemm', 'small_gemm_splitk',
    'small_gemm_batched', 'minibatch_stddev_fwd', 'minibatch_stddev_bwd', 'layer_norm_fwd', 'layer_norm_bwd', 'pixel_norm_fwd',
    'pixel_norm_bwd', 'demod_fwd', 'demod_from_wsq', 'demod_bwd', 'attn_fwd', 'attn_bwd', 'mt_adam', 'mt_ema', 'chan_scale', 'chan_dot',
    'lpips_stem_fwd', 'lpips_stem_dgrad', 'maxpool2_fwd', 'maxpool2_bwd', 'lpips_normalize', 'lpips_head_fwd', 'lpips_dist',
    'lpips_head_bwd', 'lpips_pair_head_fwd', 'crop_resize_bilinear', 'noise_reg_fwd', 'noise_reg_bwd', 'noise_normalize_', 'row_sqnorm',
    'prdc_knn', 'prdc_counts', 'vgg_stem_fwd', 'adaptive_avgpool', 'fc_stream', 'fid_moments', 'fid_finalize', 'gram', 'svm_smo',
    'svm_coef', 'conv2d', 'pool3', 'resize_bilinear', 'dex_stem_fwd', 'cls_score', 'attr_stem_fwd', 'avgpool2_act', 'attr_score',
    'conv2d_res', 'pose_stem_fwd', 'maxpool3s2p1', 'alex_stem_fwd', 'lpips_unit', 'lpips_allpairs_fwd', 'lpips_allpairs_dist',
    'conv2d_prelu', 'id_stem_fwd', 'se_excite', 'se_scale_add', 'rows_unit', 'rows_dot']


def test_roctx_ranges_behind_env_switch():
    """TE_ROCTX=1 wraps every tensor-level entry of _lib in a roctx range (operator names in rocprofv3 marker traces): the wrappers
    are the ones marked @_op where they are defined, which is every wrapper that launches"""
    import subprocess
    import sys
    code = ("from transeditor_amd import _lib; assert _lib.ROCTX and _lib.conv.__wrapped__.__name__ == 'conv' "
            "and _lib.upfirdn2d_raw.__wrapped__.__name__ == 'upfirdn2d_raw'; "
            "assert all(hasattr(f, '__wrapped__') and getattr(_lib, f.__name__) is f for f in _lib._OPS); "
            "print('ranged', ' '.join(f.__name__ for f in _lib._OPS))")
    env = dict(os.environ, TE_ROCTX='1', PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and 'ranged' in out.stdout, out.stderr
    ranged = out.stdout.split('ranged', 1)[1].split()
    assert len(_RANGED_BEFORE) == 78 and set(ranged) >= set(_RANGED_BEFORE)
    assert 'bias_act_bwd_rgb' in ranged and 'rgb_wgrad_sum_slabs' in ranged and len(set(ranged)) == len(ranged)
    from transeditor_amd import _lib
    assert not _lib.ROCTX and not hasattr(_lib.conv, '__wrapped__')
    assert [f.__name__ for f in _lib._OPS] == ranged
    assert not [f.__name__ for f in _lib._OPS if hasattr(f, '__wrapped__') or getattr(_lib, f.__name__) is not f]
    # the host-only predicates and hooks carry no range
    assert not {'wino_ok', 'wino6_form', 'wgrad_split', 'rgb_supported', 'bias_act_bwd_rgb_supported', 'fid_moments_ws_bytes',
                'fc_stream_splits', 'wgrad6_form', 'wgrad_form', 'fir_form', 'layer_norm_supported', 'small_gemm_form'} & set(ranged)


def test_fused_adam_loads_reference_style_optimizer_state():
    """the reference's torch 1.7 Adam stores `step` as a python int, and torch.load(map_location=device) moves a
    tensor `step` to the GPU; FusedAdam normalises both to a host fp32 scalar at load time (the kernel step itself is GPU-only:
    tests/test_gpu_optim.py)."""
    from transeditor_amd.optim import FusedAdam
    p = [torch.nn.Parameter(torch.randn(4, 3)), torch.nn.Parameter(torch.randn(5))]
    opt = FusedAdam(p, lr=0.002, betas=(0.0, 0.99))
    ref = torch.optim.Adam(p, lr=0.002, betas=(0.0, 0.99))
    for q in p:
        q.grad = torch.randn_like(q)
    ref.step()
    sd = ref.state_dict()
    for st in sd['state'].values():
        st['step'] = 7                                   # torch 1.7 layout: python int
    opt.load_state_dict(sd)
    for q in p:
        s = opt.state[q]['step']
        assert torch.is_tensor(s) and s.device.type == 'cpu' and s.dtype == torch.float32 and float(s) == 7.0
        assert torch.equal(opt.state[q]['exp_avg_sq'], ref.state[q]['exp_avg_sq'])
    opt.state[p[0]]['step'] = 9                          # assigned behind the optimiser's back: normalised at the next step
    FusedAdam._host_step(opt.state[p[0]])
    assert float(opt.state[p[0]]['step']) == 9.0 and torch.is_tensor(opt.state[p[0]]['step'])


def test_wgrad_group_plan_invariants():
    """te_wgrad_group_plan is host code (no GPU): NB divides B, is 1 wherever grouping must not apply (channel tails - the 16-byte
    staging path masks a tail through the end of the sample's buffer range -, a sample that already splits into chunks, too few
    blocks left), keeps every CU a block when it groups, and a group stays below the 2 GiB the zero-fill offset needs."""
    import ctypes as C
    from transeditor_amd import _lib
    L = _lib.lib()

    def plan(kind, B, Co, Ci, H, W):
        nb, s = C.c_int(0), C.c_int(0)
        assert L.te_wgrad_group_plan(kind, B, Co, Ci, H, W, C.byref(nb), C.byref(s)) == 0
        return nb.value, s.value
    for kind in (_lib.CONV_3X3, _lib.CONV_T2, _lib.CONV_1X1):
        for B in (1, 2, 8, 12, 16, 32, 64):
            for Co, Ci in ((512, 512), (512, 513), (130, 512), (128, 128), (256, 512)):
                for H in (1, 4, 8, 33, 64, 256):
                    nb, s = plan(kind, B, Co, Ci, H, H)
                    assert nb >= 1 and B % nb == 0 and s >= 1, (kind, B, Co, Ci, H, nb, s)
                    if Co % 128 or Ci % 128 or L.te_wgrad_slab_count(kind, B, Co, Ci, H, H) > 1:
                        assert nb == 1, (kind, B, Co, Ci, H, nb)
                    if nb > 1:
                        tiles = -(-Co * Ci // (128 * 64))
                        assert (B // nb) * tiles >= 256
                        biggest = max(Co * ((2 * H + 1) ** 2 if kind == _lib.CONV_T2 else H * H), Ci * H * H) * 4
                        assert nb * biggest < 2 ** 31
    assert plan(_lib.CONV_3X3, 32, 512, 512, 4, 4) == (4, 1) and plan(_lib.CONV_3X3, 16, 512, 512, 16, 16)[0] == 2
    nb, s = C.c_int(0), C.c_int(0)
    assert L.te_wgrad_group_plan(_lib.CONV_3X3, 0, 512, 512, 4, 4, C.byref(nb), C.byref(s)) != 0      # bad dims are refused


def test_minibatch_stddev_chunks_expression():
    """the recorded-backward expression of the minibatch stddev with `chunks` (Discriminator.forward(x, chunks=2): the D step's
    fake and real passes as one batch) is the per-pass statistic of model_spatial_query.py:844-852 laid end to end - and differs
    from the statistic of the joined batch"""
    import torch
    from transeditor_amd.op.stddev import _torch_expr
    from plain_torch import minibatch_stddev as plain
    torch.manual_seed(0)
    a, b = torch.randn(8, 6, 4, 4, dtype=torch.float64), torch.randn(8, 6, 4, 4, dtype=torch.float64)
    joint = _torch_expr(torch.cat([a, b]), 4, 1, chunks=2)
    assert torch.allclose(joint, torch.cat([plain(a, 4), plain(b, 4)]), rtol=1e-12, atol=1e-14)
    assert not torch.allclose(joint, plain(torch.cat([a, b]), 4))
    assert torch.equal(_torch_expr(a, 4, 1, chunks=1), plain(a, 4))


def test_packed_weight_cache_refresh_logic(monkeypatch):
    """host logic of the packed-weight cache (op/modconv.py) with the packing launches replaced by fakes: hits while the version
    counter stands, ONE multi-tensor refresh of exactly the stale entries after an optimiser step (into fresh buffers), entries of partial
    views dropped, temporaries never cached"""
    import torch
    from transeditor_amd import _lib
    from transeditor_amd.op import weight_cache as mc
    calls = {'single': 0, 'multi': []}

    def conv_pack(w, kind, wscale=1.0):
        calls['single'] += 1
        return (w.detach().flatten() * wscale + kind).clone()

    def conv_pack2(w, ka, kb, wscale=1.0):
        return conv_pack(w, ka, wscale), conv_pack(w, kb, wscale)

    def conv_pack_multi(jobs):
        calls['multi'].append(len(jobs))
        for wp, w, kind, wscale in jobs:
            wp.copy_(w.flatten() * wscale + kind)
    monkeypatch.setattr(_lib, 'conv_pack', conv_pack)
    monkeypatch.setattr(_lib, 'conv_pack2', conv_pack2)
    monkeypatch.setattr(_lib, 'conv_pack_multi', conv_pack_multi)
    p5 = torch.nn.Parameter(torch.randn(1, 4, 3, 3, 3))          # ModulatedConv2d layout: the op sees weight[0]
    p4 = torch.nn.Parameter(torch.randn(4, 3, 1, 1))
    p2 = torch.nn.Parameter(torch.randn(2, 4, 3, 3, 3))          # a PARTIAL view of it is cached but cannot be refreshed in bulk
    cache = {}
    with mc.packed_weights_cache(cache):
        a = mc.packed(p5[0], 0, 0.5)
        mc.packed2(p4, 0, 1, 2.0)
        mc.packed(p2[1], 0, 1.0)
        assert mc.packed(p5[0], 0, 0.5) is a and calls['single'] == 4 and len(cache) == 4
        mc.packed(torch.randn(4, 3, 3, 3), 0, 1.0)                # a temporary: packed, not cached
        assert len(cache) == 4 and calls['single'] == 5
        assert mc.refresh_packed_weights(cache) == 0 and calls['multi'] == [0]
        with torch.no_grad():
            for p in (p5, p4, p2):
                p.mul_(2.0)                                       # "optimiser step": version counters move
        assert mc.refresh_packed_weights(cache) == 3 and calls['multi'][-1] == 3      # p5 (1 layout) + p4 (2 layouts); the partial view is dropped
        assert len(cache) == 3
        a_old = a.clone()
        a2 = mc.packed(p5[0], 0, 0.5)                             # a hit again, on a NEW buffer: the old layout (possibly still
        assert a2 is not a and torch.equal(a, a_old)              # held by an autograd node) is left untouched
        assert torch.equal(a2, p5.detach()[0].flatten() * 0.5) and mc.packed(p5[0], 0, 0.5) is a2
        assert calls['single'] == 5
        mc.packed(p2[1], 0, 1.0)                                  # the dropped entry is repacked at its next use
        assert calls['single'] == 6 and len(cache) == 4


def test_forward_plans_and_packs_once(monkeypatch, libpath):
    """host logic of op/modconv.packed_route / _fwd_raw with the launches replaced by recording fakes, on two shapes that take a split
    kernel on both sides (tests/conv_routes.py: '3x3_w6_both', 'down_s2s6_t2s6'): (a) a forward that will meet a data gradient packs
    both layouts in ONE launch and keeps (data-gradient layout, its kind), which _dgrad_raw(wp=...) launches even after the switches
    moved; (b) a no-grad forward on a parameter inside an open packed_weights_cache packs the data-gradient layout ahead; (c) any other
    forward packs the forward layout alone; (d) every launch runs the kind the selector names"""
    import conv_routes as cr
    from transeditor_amd import _lib
    from transeditor_amd.op import modconv as mc
    from transeditor_amd.op.weight_cache import packed_weights_cache
    log = []

    def conv_pack(w, kind, wscale=1.0):
        log.append(('pack', kind))
        return torch.full((1,), float(kind))

    def conv_pack2(w, ka, kb, wscale=1.0):
        log.append(('pack2', ka, kb))
        return torch.full((1,), float(ka)), torch.full((1,), float(kb))

    def conv(x, wp, kind, M, H, W, *a, **k):
        log.append(('conv', kind, int(wp[0])))
        return torch.empty(_lib.conv_out_shape(kind, x.shape[0], M, H, W))
    monkeypatch.setattr(_lib, 'conv_pack', conv_pack)
    monkeypatch.setattr(_lib, 'conv_pack2', conv_pack2)
    monkeypatch.setattr(_lib, 'conv', conv)
    for op, (B, K, M, H, W) in (('3x3', (1, 64, 64, 8, 32)), ('down', (1, 64, 64, 8, 16))):
        w = torch.nn.Parameter(torch.empty(M, K, 3, 3))
        x = torch.empty(B, K, H, W) if op == '3x3' else torch.empty(B, K, 2 * H + 1, 2 * W + 1)
        (pf, cf), (pb, cb) = mc.fwd_kinds(op, B, w, H, W), mc.bwd_kinds(op, B, w, H, W)
        assert (cr.PACK_NAMES[pf], cr.CONV_NAMES[cf]) == cr.BY_NAME['3x3_w6_both' if op == '3x3' else 'down_s2s6_t2s6'].fwd
        assert cf != cb or pf != pb
        # (a), through the helper and through _fwd_raw
        del log[:]
        wp, ck, (wpb, ckb) = mc.packed_route(op, B, w, H, W, 0.5, True)
        assert log == [('pack2', pf, pb)] and (int(wp[0]), ck, int(wpb[0]), ckb) == (pf, cf, pb, cb)
        del log[:]
        y, kept = mc._fwd_raw(x, w, op, wscale=0.5, with_bwd_pack=True)
        assert log == [('pack2', pf, pb), ('conv', cf, pf)] and (int(kept[0][0]), kept[1]) == (pb, cb)          # (d)
        del log[:]
        with cr.switches(split_bf16=False):                      # the kind decided at forward time is the one launched
            assert mc.bwd_kinds(op, B, w, H, W) != (pb, cb)
            mc._dgrad_raw(y, w, op, wscale=0.5, wp=kept)
        assert log == [('conv', cb, pb)]
        del log[:]
        mc._dgrad_raw(y, w, op, wscale=0.5)                       # (without a kept pair: planned and packed now)
        assert log == [('pack', pb), ('conv', cb, pb)]
        # (b)
        del log[:]
        cache = {}
        with packed_weights_cache(cache), torch.no_grad():
            mc._fwd_raw(x, w, op, wscale=0.5)
        assert log == [('pack2', pf, pb), ('conv', cf, pf)] and sorted(k[2] for k in cache) == sorted((pf, pb))
        # (c): no cache open; a cache open but a forward that records; the helper asked for one layout
        del log[:]
        with torch.no_grad():
            mc._fwd_raw(x, w, op, wscale=0.5)
        with packed_weights_cache({}):
            mc._fwd_raw(x, w, op, wscale=0.5)
        assert log == [('pack', pf), ('conv', cf, pf)] * 2
        del log[:]
        assert mc.packed_route(op, B, w, H, W, 0.5, False)[1:] == (cf, None) and log == [('pack', pf)]


def test_convolution_form_selection_is_a_pure_function_of_the_shape(libpath):
    """op/modconv.fwd_kinds / bwd_kinds (no GPU): split-bf16 Winograd where te_conv_wino6_supported says so, fp32 Winograd where only
    te_conv_wino_supported does, the direct kernels elsewhere; TE_SPLIT_BF16 / USE_WINOGRAD switch the forms off in that order"""
    from transeditor_amd import _lib
    from transeditor_amd.op import modconv
    w = lambda co, ci: torch.empty(co, ci, 3, 3)
    assert modconv.fwd_kinds('3x3', 16, w(128, 128), 256, 256) == (_lib.PACK_W6FWD, _lib.CONV_3X3W6)
    assert modconv.bwd_kinds('3x3', 16, w(256, 512), 64, 64) == (_lib.PACK_W6DGRAD, _lib.CONV_3X3W6)
    assert modconv.fwd_kinds('3x3', 4, w(32, 32), 1024, 1024) == (_lib.PACK_WFWD, _lib.CONV_3X3W)
    assert modconv.fwd_kinds('3x3', 16, w(512, 512), 16, 16) == (_lib.PACK_W6FWD, _lib.CONV_3X3W6)        # round 6: two samples side by side
    assert modconv.fwd_kinds('3x3', 15, w(512, 512), 16, 16) == (_lib.PACK_FWD, _lib.CONV_3X3)            # (odd batch), small batches, smaller images: direct kernel
    assert modconv.fwd_kinds('3x3', 8, w(512, 512), 16, 16) == (_lib.PACK_FWD, _lib.CONV_3X3)
    assert modconv.fwd_kinds('3x3', 16, w(512, 512), 8, 8) == (_lib.PACK_FWD, _lib.CONV_3X3)
    # (round 5) the strided kind on the bf16 pipe where te_conv_s2s6_supported says so: the up-sampling layers' data gradient and the
    # discriminator's down-sampling convolutions from 16 x 16 outputs up; smaller images stay on the fp32 kernel
    assert modconv.fwd_kinds('up', 16, w(256, 512), 64, 64) == (_lib.PACK_T6FWD, _lib.CONV_T2S6)
    assert modconv.fwd_kinds('up', 16, w(512, 512), 8, 8) == (_lib.PACK_FWD, _lib.CONV_T2)
    assert modconv.bwd_kinds('down', 32, w(256, 128), 128, 128) == (_lib.PACK_T6SWAP, _lib.CONV_T2S6)
    assert modconv.bwd_kinds('up', 16, w(256, 512), 64, 64) == (_lib.PACK_S6SWAP, _lib.CONV_S2S6)
    assert modconv.fwd_kinds('down', 32, w(256, 128), 128, 128) == (_lib.PACK_S6FWD, _lib.CONV_S2S6)
    assert modconv.fwd_kinds('down', 32, w(512, 512), 8, 8) == (_lib.PACK_FWD, _lib.CONV_S2)
    assert modconv.bwd_kinds('up', 16, w(512, 512), 4, 4) == (_lib.PACK_SWAP, _lib.CONV_S2)
    old = modconv.USE_SPLIT_BF16, modconv.USE_WINOGRAD
    try:
        modconv.USE_SPLIT_BF16 = False
        assert modconv.fwd_kinds('3x3', 16, w(128, 128), 256, 256) == (_lib.PACK_WFWD, _lib.CONV_3X3W)
        assert _lib.wgrad_split() == 0               # ONE switch: the weight-gradient kernels follow the Python flag
        modconv.USE_WINOGRAD = False
        assert modconv.fwd_kinds('3x3', 16, w(128, 128), 256, 256) == (_lib.PACK_FWD, _lib.CONV_3X3)
    finally:
        modconv.USE_SPLIT_BF16, modconv.USE_WINOGRAD = old
    assert _lib.wgrad_split() == (1 if old[0] else 0)


def test_load_checkpoint_into_is_all_or_nothing():
    """train_step.load_checkpoint_into validates its arguments BEFORE loading anything (the reference's restore,
    train_spatial_query.py:475-492, is all-or-nothing): a partial set of training objects or a file with some but not all training
    entries raises and leaves every module untouched; a 'g_ema'-only file loads the EMA generator alone; a full checkpoint into g_ema only warns."""
    import warnings

    import torch
    from transeditor_amd.train_step import load_checkpoint_into
    mk = lambda: torch.nn.Linear(3, 2)
    src = {k: mk() for k in ('g_ema', 'g', 'd')}
    opt = {k: torch.optim.Adam(src[k].parameters()) for k in ('g', 'd')}
    full = {'g_ema': src['g_ema'].state_dict(), 'g': src['g'].state_dict(), 'd': src['d'].state_dict(),
            'g_optim': opt['g'].state_dict(), 'd_optim': opt['d'].state_dict()}
    ema, g, d = mk(), mk(), mk()
    before = ema.weight.clone()
    go, do = torch.optim.Adam(g.parameters()), torch.optim.Adam(d.parameters())
    with pytest.raises(ValueError):
        load_checkpoint_into(full, ema, generator=g)                    # partial set of training objects
    with pytest.raises(KeyError):
        load_checkpoint_into({k: full[k] for k in ('g_ema', 'g', 'd')}, ema, g, d, go, do)   # neither a training nor a g_ema-only file
    assert torch.equal(ema.weight, before)                                  # nothing was loaded on the failed attempts
    gw = g.weight.clone()
    with pytest.raises(KeyError):                    # a g_ema-only file into a TRAINING restore: the reference's ckpt['g'] raises too (:487)
        load_checkpoint_into({'g_ema': src['d'].state_dict()}, ema, g, d, go, do)
    assert torch.equal(ema.weight, before)
    assert load_checkpoint_into({'g_ema': src['d'].state_dict()}, ema, g, d, go, do, g_ema_only_ok=True) is None   # knowingly: EMA alone
    assert torch.equal(ema.weight, src['d'].weight) and torch.equal(g.weight, gw)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        load_checkpoint_into(full, ema)
    assert any('g_ema only' in str(r.message) for r in rec)
    assert torch.equal(ema.weight, src['g_ema'].weight)
    load_checkpoint_into(full, ema, g, d, go, do)
    assert torch.equal(g.weight, src['g'].weight) and torch.equal(d.weight, src['d'].weight)
