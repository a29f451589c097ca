"""fp16 / bf16 sparse 3D convolution on the MI355X (csrc/sparse_conv_16.hip): the cases of tests/sparse_conv_16_cases.py on cuda:0,
through the helpers of tests/test_cpu_sparse_conv_16.py.  The 16-bit outputs lie within E + u16 (|want| + E) + s of the fp64 dense-conv3d
oracle on the rounded operands, the fp32 weight and bias gradients within (L + 2) 2^-24 A, and all four are bit-identical from run to
run; the 20 000-row sweeps; the C entries on sentinel-filled buffers with guard bands, aligned and shifted by 2 bytes (all bases, and one
operand at a time), the dense() entries likewise; non-finite inputs and sums beyond the range; the static form of a two-layer stack
recorded and replayed in one graph; MlvlSparseEncoder in bf16 layer by layer; dense(); the device guard."""
import numpy as np
import pytest
import torch

import mmdet3d_gaussian_amd as amd
import sparse_conv_16_cases as c16
import sparse_conv_ref as ref
from mmdet3d_gaussian_amd import _lib
from mmdet3d_gaussian_amd.sparse_conv import _backward_entries
from sparse_twins import refuse_twins
from test_cpu_sparse_conv import ENC_B, ENC_SHAPES, SWEEPS, build_encoder, check_nonfinite_containment, encoder_inputs, run_index
from test_cpu_sparse_conv_16 import KINDS, check_dense_16, check_modules_16, check_range_16, check_values_16, convs_of, run_values_16

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = -77.0           # the sentinel of the guard test: exact in fp16 and in bf16, far outside every bound


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', c16.VALUE_CASES)
def test_values_within_the_bounds_and_the_same_bits_from_run_to_run(name, kind):
    got = run_values_16(name, DEV, kind)
    check_values_16(name, DEV, kind, got)                         # the device's results; the twin's are held to the same bound on the CPU
    again = run_values_16(name, DEV, kind)
    for k in ('out', 'gx', 'gw', 'gb'):
        if got[k] is not None:
            assert got[k].tobytes() == again[k].tobytes(), f'{name} {kind}: {k} differs from run to run'


@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_channel_tiles_c24_40', 'subm_channel_tiles_c32_32'])
def test_the_device_and_the_twin_each_lie_within_the_bound(name):
    for kind in KINDS:
        check_values_16(name, DEV, kind)
        check_values_16(name, 'cpu', kind)


@pytest.mark.parametrize('name', SWEEPS)
def test_sweep_of_20000_rows_in_bf16(name):
    """about 20 000 rows over 3 samples at 16 -> 32: 157 workgroups of the forward kernel, 64 partial sums per offset in the weight gradient"""
    index = run_index(ref.case_of(name), DEV)
    got = run_values_16(name, DEV, 'bf16', index)
    check_values_16(name, DEV, 'bf16', got)
    again = run_values_16(name, DEV, 'bf16', index)
    for k in ('out', 'gx', 'gw', 'gb'):
        assert got[k].tobytes() == again[k].tobytes(), f'{name}: {k} differs from run to run'


WIDE = 'wide_subm_c65_130'   # 200 rows at 65 -> 130: two input and three output tiles of 64, so blockIdx.z is split with tiles_co = 3
WGRAD_CASES = tuple(dict.fromkeys(list(c16.VALUE_CASES) + list(c16.DEAD_TILE_CASES))) + (WIDE,)


def wgrad_operands(name):
    """-> (case, X, gY): fp32 operands on the device, fixed by the case"""
    if name != WIDE:
        X, _, _, gY = c16.operands(name)
        return c16.case_of(name), torch.from_numpy(X).to(DEV), torch.from_numpy(gY).to(DEV)
    rng = np.random.default_rng(26)
    case = ref._case(ref.random_coors(rng, 200, (9, 12, 10), 2), (9, 12, 10), 2, 'subm', 65, 130)
    return case, torch.from_numpy(rng.standard_normal((200, 65)).astype(np.float32)).to(DEV), \
        torch.from_numpy(rng.standard_normal((200, 130)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize('name', WGRAD_CASES)
def test_the_16_bit_weight_gradient_is_the_fp32_entry_on_the_widened_operands_bit_for_bit(name):
    """gd3d_sparse_conv_backward_weight_16 against gd3d_sparse_conv_backward_weight on the same 16-bit operands widened to fp32 (exact):
    grad_weight and grad_bias are equal bit for bit, in fp16 and in bf16, with a bias gradient and without.  One source computes both
    (csrc/sparse_conv_wgrad.hip): the tiles, the 32-row steps, the chunks and the order of every sum are the same by construction."""
    case, X, gY = wgrad_operands(name)
    index = run_index(case, DEV)
    w = torch.empty((index.nbr.size(1), case['cin'], case['cout']), device=DEV)       # its shape alone is read: no input gradient is asked for
    pairs = bool(((index.nbr >= 0) & (torch.arange(index.nbr.size(0), device=DEV) < index.num[0])[:, None]).any())
    for kind in KINDS:
        dtype = c16.DTYPES[kind]
        x16, g16 = X.to(dtype), gY.to(dtype)
        for has_bias in (True, False):
            run = lambda x, g, dt: _backward_entries(x, w, g, index.nbr, index.nbr_t, index.num, case['subm'], False, True, has_bias, dt)[1:]
            gw16, gb16 = run(x16, g16, dtype)
            gw32, gb32 = run(x16.float(), g16.float(), None)
            assert gw16.dtype == torch.float32 and torch.equal(gw16, gw32), f'{name} {kind}: grad_weight differs from the fp32 entry'
            assert bool(gw16.any()) == pairs and torch.isfinite(gw16).all(), f'{name} {kind}: grad_weight'
            if has_bias:
                assert gb16.dtype == torch.float32 and torch.equal(gb16, gb32), f'{name} {kind}: grad_bias differs from the fp32 entry'
                assert bool(gb16.any()) == pairs
            else:
                assert gb16 is None and gb32 is None


def run_c_entries_between_bands(name, kind, shift):
    """the 16-bit C entry points on sentinel-filled buffers with a guard band either side of every output and of the workspace: every
    element of every output is written, the bands stay untouched.  shift: elements (of 2 bytes) past an aligned address, for the gathered
    operand ('src': features, grad_out), for 'weight' and for the 16-bit outputs ('out': out, grad_features).  -> the four results"""
    dtype, code = c16.DTYPES[kind], {'fp16': 1, 'bf16': 2}[kind]
    case, want = ref.case_of(name), ref.expected_index(name)
    X, W, bias, gY = (None if a is None else torch.from_numpy(a).to(DEV) for a in ref.operands(name))
    index = run_index(case, DEV)
    N, (K, Cin, Cout), R = len(X), W.shape, len(want['nbr'])
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    G, band = 64, 4096

    def shifted(t, by):                                           # a 16-bit copy whose base is `by` elements past an aligned allocation
        buf = torch.empty(t.numel() + 8, dtype=dtype, device=DEV)
        buf[by:by + t.numel()] = t.to(dtype).flatten()
        assert buf.data_ptr() % 16 == 0
        return buf, buf.data_ptr() + 2 * by
    (x16, x_at), (w16, w_at), (g16, g_at) = shifted(X, shift['src']), shifted(W, shift['weight']), shifted(gY, shift['src'])
    sizes = dict(out=(R * Cout, dtype), gx=(N * Cin, dtype), gw=(K * Cin * Cout, torch.float32), gb=(Cout, torch.float32))
    bufs = {k: torch.full((n + 2 * G,), S, dtype=dt, device=DEV) for k, (n, dt) in sizes.items()}
    off = dict(out=G + shift['out'], gx=G + shift['out'], gw=G, gb=G)
    at = lambda k: bufs[k].data_ptr() + off[k] * bufs[k].element_size()
    nbytes = lib.gd3d_sparse_conv_backward_weight_workspace_bytes(R, K, Cin, Cout)
    assert nbytes % 256 == 0
    work = torch.full((nbytes + 2 * band,), 0x5a, dtype=torch.uint8, device=DEV)
    assert (work.data_ptr() + band) % 256 == 0
    nbr, nbr_t, num = index.nbr.data_ptr(), None if case['subm'] else index.nbr_t.data_ptr(), index.num.data_ptr()
    _lib.check(lib.gd3d_sparse_conv_forward_16(x_at, w_at, None if bias is None else bias.data_ptr(), nbr, num, N, R, K, Cin, Cout, code,
                                               at('out'), stream), 'gd3d_sparse_conv_forward_16')
    _lib.check(lib.gd3d_sparse_conv_backward_input_16(g_at, w_at, nbr if case['subm'] else nbr_t, int(case['subm']), N, R, K, Cin, Cout, code,
                                                      at('gx'), stream), 'gd3d_sparse_conv_backward_input_16')
    _lib.check(lib.gd3d_sparse_conv_backward_weight_16(x_at, g_at, nbr, num, N, R, K, Cin, Cout, code, work.data_ptr() + band, at('gw'),
                                                       None if bias is None else at('gb'), stream), 'gd3d_sparse_conv_backward_weight_16')
    torch.cuda.synchronize()
    got = {}
    for k, (n, dt) in sizes.items():
        t, o = bufs[k], off[k]
        assert (t[:o] == S).all() and (t[o + n:] == S).all(), f'{k}: a guard band was written'
        got[k] = t[o:o + n].float().cpu().numpy()
    assert (work[:band] == 0x5a).all() and (work[-band:] == 0x5a).all(), 'a workspace band was written'
    o64 = c16.expected_values(name, kind)[0]
    got = {k: (None if o64[k] is None else got[k].reshape(o64[k].shape)) for k in sizes}
    check_values_16(name, DEV, kind, got)                         # every element written: no sentinel survives the bound
    return got


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted_2_bytes'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', c16.GUARD_CASES)
def test_nothing_is_written_beyond_the_outputs_and_the_workspace(name, kind, shift):
    """with every 16-bit base shifted by one element (2 bytes) the element-wise loads and stores give the same values"""
    run_c_entries_between_bands(name, kind, dict(src=shift, weight=shift, out=shift))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_rows_tile_plus_1', 'down_7x11x13_c16_32'])
def test_one_misaligned_operand_at_a_time_gives_the_aligned_calls_bits(name, kind):
    """the gather, the weight staging and the stores each fall back to their element-wise form on their own: the same arithmetic, so
    the same bits as the call on aligned operands (include/gd3d.h)"""
    aligned = run_c_entries_between_bands(name, kind, dict(src=0, weight=0, out=0))
    for which in ('src', 'weight', 'out'):
        got = run_c_entries_between_bands(name, kind, dict(dict(src=0, weight=0, out=0), **{which: 1}))
        for k in ('out', 'gx', 'gw', 'gb'):
            assert got[k].tobytes() == aligned[k].tobytes(), f'{name} {kind}: {k} changes with a misaligned {which}'


@pytest.mark.parametrize('shift', [0, 1], ids=['aligned', 'shifted_2_bytes'])
@pytest.mark.parametrize('C', [3, 4], ids=['odd_count', 'even_count'])
def test_dense_16_entries_between_bands(C, shift):
    """gd3d_sparse_to_dense_16 / _backward_16 on banded buffers, C * D * H * W = 315 (odd) and 420 (even) elements from an aligned base
    and from one 2 bytes past it: the fill's tail-only, neither, head-only and head-and-tail forms.  Every element between the bands
    is written and equals the fp32 route's; the bands stay untouched."""
    shape, B, G = (3, 5, 7), 1, 64
    rng = np.random.default_rng(25)
    rows = np.concatenate([ref.random_coors(rng, 20, shape, B), np.array([[-1, -1, -1, -1], [1, 0, 0, 0], [0, 3, 0, 0]], np.int32)])
    coors, N, n = torch.from_numpy(rows).to(DEV), len(rows), C * B * shape[0] * shape[1] * shape[2]
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for dtype in c16.DTYPES.values():
        feats = torch.from_numpy(rng.standard_normal((N, C)).astype(np.float32)).to(DEV).to(dtype)
        want = amd.sparse_to_dense(feats.float(), coors, shape, B).to(dtype)
        dense = torch.full((n + 2 * G,), S, dtype=dtype, device=DEV)
        lo = G + shift
        assert dense.data_ptr() % 16 == 0 and (dense.data_ptr() + 2 * lo) % 4 == 2 * shift
        _lib.check(lib.gd3d_sparse_to_dense_16(feats.data_ptr(), coors.data_ptr(), N, C, B, *shape, dense.data_ptr() + 2 * lo, stream), 'gd3d_sparse_to_dense_16')
        torch.cuda.synchronize()
        assert (dense[:lo] == S).all() and (dense[lo + n:] == S).all(), 'a guard band was written'
        assert torch.equal(dense[lo:lo + n].reshape(want.shape), want) and want.any()
        gx = torch.full((N * C + 2 * G,), S, dtype=dtype, device=DEV)
        _lib.check(lib.gd3d_sparse_to_dense_backward_16(dense.data_ptr() + 2 * lo, coors.data_ptr(), N, C, B, *shape, gx.data_ptr() + 2 * lo, stream),
                   'gd3d_sparse_to_dense_backward_16')
        torch.cuda.synchronize()
        assert (gx[:lo] == S).all() and (gx[lo + N * C:] == S).all(), 'a guard band was written'
        back = gx[lo:lo + N * C].reshape(N, C)
        assert torch.equal(back[:20], feats[:20]) and not back[20:].any()     # the gather of what was scattered; inactive rows zero


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', ['subm_9x12x10_c4_16', 's2p1_9x12x10_c5_16'])
def test_a_non_finite_value_reaches_only_what_reads_it(name, kind):
    check_nonfinite_containment(name, DEV, c16.DTYPES[kind])


@pytest.mark.parametrize('kind', KINDS)
def test_a_sum_beyond_the_range_is_inf_not_the_largest_finite_value(kind):
    check_range_16(DEV, kind)


def test_modules_equal_the_functional_form():
    check_modules_16(DEV)


def test_dense_of_16_bit_features_equals_the_upcast_route():
    check_dense_16(DEV)


def test_static_form_of_a_two_layer_stack_under_graph_capture():
    """SparseConv3d(k3 s2 p1, max_out) -> SubMConv3d, both in bf16, forward and backward, on the static rows of a voxelization (tail rows
    -1): recorded on a single stream in ONE graph, replayed on fresh coordinates, features and upstream gradient in the static buffers,
    and compared with the eager run of the same inputs bit for bit"""
    shape, B, N, MO = (9, 12, 10), 2, 200, 230        # 248 outputs of the first 180 rows (capped), 216 of the fresh 120 (a tail)
    rng = np.random.default_rng(17)

    def rows(n_active):
        c = np.full((N, 4), -1, np.int32)
        c[:n_active] = ref.random_coors(rng, n_active, shape, B)
        return torch.from_numpy(c)
    torch.manual_seed(18)
    down = amd.SparseConv3d(16, 32, 3, 2, 1, bias=True, max_out=MO, compute_dtype=torch.bfloat16).to(DEV)
    subm = amd.SubMConv3d(32, 32, 3, bias=False, compute_dtype=torch.bfloat16).to(DEV)
    params = [down.weight, down.bias, subm.weight]
    coors, feats, gy = rows(180).to(DEV), torch.randn(N, 16, device=DEV).requires_grad_(True), torch.randn(MO, 32, device=DEV).bfloat16()

    def step():
        y = subm(down(amd.SparseConvTensor(feats, coors, shape, B)))
        return [y.indices, y.features] + list(torch.autograd.grad(y.features, [feats] + params, gy))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = [t.clone() for t in step()]                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(captured, warm):
        assert torch.equal(got, want)
    with torch.no_grad():
        coors.copy_(rows(120))
        feats.copy_(torch.randn(N, 16, device=DEV))
        gy.copy_(torch.randn(MO, 32, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    assert captured[1].dtype == torch.bfloat16 and captured[2].dtype == torch.float32 and captured[3].dtype == torch.float32
    assert not torch.equal(eager[0], warm[0]) and not torch.equal(eager[1], warm[1])
    for got, want in zip(captured, eager):
        assert torch.equal(got, want)
    kept = int(ref.index_ref(coors.cpu().numpy(), shape, B, *ref.GEOMS['s2p1'], max_out=MO)['num'][0])
    assert 0 < kept < MO and captured[1][:kept].any() and not captured[1][kept:].any(), 'tail rows are zero, bias or not'
    assert not captured[2][120:].any() and all(torch.isfinite(t).all() for t in captured[1:])


def test_mlvl_sparse_encoder_in_bf16_follows_the_per_layer_fp64_oracle():
    """MlvlSparseEncoder(compute_dtype=bf16) on the smallest grid: every conv layer's output within that layer's bound of the fp64 oracle
    evaluated on the layer's own 16-bit input; spatial_features is bf16; one backward reaches every parameter with a finite fp32 gradient"""
    grid = min(ENC_SHAPES, key=lambda s: s[0] * s[1] * s[2])
    coors, feats = encoder_inputs(grid)
    enc = build_encoder(DEV, grid)
    ref_state = enc.state_dict()
    torch.manual_seed(6)
    enc = amd.MlvlSparseEncoder(in_channels=4, sparse_shape=list(grid), order=('conv', 'norm', 'act'), compute_dtype=torch.bfloat16).to(DEV).eval()
    enc.load_state_dict(ref_state)
    seen = []
    hooks = [m.register_forward_hook(lambda mod, args, out: seen.append((mod, args[0].features.detach(), args[0].indices, list(args[0].spatial_shape),
                                                                            out.features.detach()))) for m in convs_of(enc)]
    got = enc(torch.from_numpy(feats).to(DEV), torch.from_numpy(coors).to(DEV), ENC_B)
    for h in hooks:
        h.remove()
    assert len(seen) == len(convs_of(enc)) == 12
    worst = 0.0
    for conv, x, c, shape, y in seen:
        assert y.dtype == torch.bfloat16
        idx = ref.index_ref(c.cpu().numpy(), shape, ENC_B, conv.kernel_size, conv.stride, conv.padding, conv.subm)
        if len(idx['nbr']) == 0:                                  # the kernel does not fit the grid: no output cell
            assert y.shape[0] == 0
            continue
        X = x.to(torch.bfloat16).double().cpu().numpy()
        W = conv.weight.detach().to(torch.bfloat16).double().cpu().numpy().reshape(-1, conv.in_channels, conv.out_channels)
        zeros = np.zeros((len(idx['nbr']), conv.out_channels))
        want = ref.sparse_oracle(idx, X, W, None, zeros)['out']
        A = ref.sparse_oracle(idx, np.abs(X), np.abs(W), None, zeros)['out']
        L = ref.term_counts(idx, len(X), conv.in_channels, conv.out_channels, False)['out']
        ok, ratio = c16.within_bound_16(y.float().cpu().numpy(), want, A, L, 'bf16')
        worst = max(worst, ratio)
        assert ok, f'{conv}: the output misses its bound: worst |ours - o64| / A = {ratio:.3e}'
    print(f'MlvlSparseEncoder in bf16 on {DEV}: worst |ours - o64| / A over the conv layers {worst:.3e}')
    sp = got['spatial_features']
    assert sp.dtype == torch.bfloat16 and sp.dim() == 4 and sp.shape[0] == ENC_B
    assert all(f.features.dtype == torch.bfloat16 for f in got['encode_features'])
    loss = sp.float().square().sum() + sum(f.features.float().square().sum() for f in got['encode_features'])
    loss.backward()
    for n, p in enc.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), n
    assert any(p.grad.abs().sum() > 0 for n, p in enc.named_parameters() if n.endswith('0.weight'))


def test_device_tensors_never_reach_a_twin(monkeypatch):
    """a `_cpu` twin called with the address of device memory would fault the process: every 16-bit twin is replaced by a function that
    raises, and the whole 16-bit surface runs on cuda:0"""
    refuse_twins(monkeypatch, lambda name: name.endswith('_16_cpu'))
    with pytest.raises(AssertionError, match='_16_cpu was called'):      # the replacement is in place: CPU tensors do reach it
        run_values_16('subm_rows_1', 'cpu', 'bf16')
    check_values_16('subm_9x12x10_c4_16', DEV, 'fp16')
    check_dense_16(DEV)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_a_call_on_another_devices_tensors_leaves_the_callers_device_current():
    torch.cuda.set_device(0)
    name = 's2p1_9x12x10_c5_16'
    want = run_values_16(name, 'cuda:0', 'bf16')
    got = run_values_16(name, 'cuda:1', 'bf16')
    assert torch.cuda.current_device() == 0
    for k in ('out', 'gx', 'gw', 'gb'):
        assert got[k].tobytes() == want[k].tobytes(), k
    check_dense_16('cuda:1')
    assert torch.cuda.current_device() == 0
