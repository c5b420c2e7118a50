"""
Every output element of the fp32 GEMM family (csrc/gemm_f32.hip, csrc/gemm_atb.hip: v_mfma_f32_32x32x2_f32) against float64,
each within its own allowance gamma u m (tests/elementwise.py::gemm_reference), on every path `launch_gemm` can take:

    a. every kernel of `pick_gemm` through empose_linear_f32_ex -- the 64x64 / 64x128 / 128x64 tiles, the 8-wave 256x128
       tile, the hand-pipelined 256x256 tile (which no other test reaches), split-K with four and with eight waves, the
       few-rows kernel with 4 / 8 / 12 / 16 rows -- each with every epilogue form (none; scale + shift; PReLU with a
       negative and a positive slope; PReLU + residual; residual-then-ReLU with and without a residual), ragged in M, N and
       K, every leading dimension padded and different, 1e18 behind the K columns of both operands, and the padding and a
       guard row of C asserted untouched to the bit.  Each case names the kernel it is meant to reach and first asserts
       that empose_profile_gemm_kernel_name agrees, so a retuned `pick_gemm` cannot silently empty the grid;
    b. the two-problem launches of the layer-by-layer update MLPs (mlp_fused = 0) at T = 16379: the 256x256 tile with
       count 2 (ROLE 0 at the ragged K = 296, ROLE 1 at K = 512), the 8-wave tile under gemm_wide = 0, the 66- / 10-column
       output launch, and a skip-connection net for the wide tile's residual epilogue;
    c. empose_gemm_strided_f32 in its four <A_KC, W_KC> instantiations, incl. K % 4 != 0 and unaligned bases;
    d. empose_gemm_atb_f32, result and column sums, at the shapes of test_hip_parity.py::test_gemm_atb_vs_float64.

Measured on the MI355X against float64, the worst error over every element of every case of this module in units of the
allowance at gamma = 1 (the gamma the element would have needed; for a. and c. the allowance of
elementwise.gemm_reference -- root-sum-square over the partial sums of the k-ordered chain + the worst-case epilogue --,
for b. that of eval_mlp_reference, for d. the worst case u |A|^T |B| and u sum |a|: its reductions are split over rows):
    gemm_wide_f32_kernel<0>       2.81 (K = 64), 2.56 (68), 2.52 (92), 2.41 (96), 2.53 (100), 2.49 (3841 x 4096 x 100)
    256 x 128 tile (8 waves)      2.25 (1930 x 4000 x 100), 2.53 (the wide shape under gemm_wide = 0)
    128 x 64 tile                 1.51
    64 x 128 tile                 1.88 (61 x 130 x 44), 2.32 (2100 x 1000 x 72)
    64 x 64 tile                  0.71 (1 x 4 x 4), 1.70 (40 x 50 x 36), 2.12 (1000 x 512 x 144)
    split-K, 4 waves              2.01 (33 x 95 x 68), 2.27 (300 x 1000 x 1024)
    split-K, 8 waves              1.50, 1.83; beside the few-rows condition 0.95, 1.36, 1.26
    few-rows, 4 / 8 / 12 / 16     0.53, 0.58, 0.73, 0.46; K = 2308: 0.51
    update nets, layer by layer   wide tile 2.48, with skip connections 2.24; 8-wave tile the same two figures
    strided split-K               2.92 (384 x 512 x 513, A gathered, W K-contiguous); the other shapes 1.7 .. 2.5
    A^T B                         3.14 (130 x 200 x 320); column sums 0.92
The worst is 3.14, so GAMMA_GEMM = 8: the smallest power of two that leaves the factor 2 for other summation orders and
other machines, and the family's cap.  With the coarser accumulation terms tried first the same kernels needed 6.82 (worst
case u |A| |W|^T, wide tile at K = 96) and 5.15 (order-averaged root-sum-square): see elementwise.gemm_reference.
No defect showed up: every kernel within its allowance on every path, the padding of C and its guard row untouched.
"""
import pytest
import torch

from em_pose_amd import _lib
from tests import elementwise as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAMMA = E.GAMMA_GEMM

# names as empose_profile_gemm_kernel_name (and a profiler) prints them
KERNEL_NAMES = {
    'WIDE': 'gemm_wide_f32_kernel<0>',
    'LARGE': 'gemm_tn_f32_kernel<Cfg<4,2,2,2,32,false>,0>',
    'S21': 'gemm_tn_f32_kernel<Cfg<2,2,2,1,32,false>,0>',
    'S12': 'gemm_tn_f32_kernel<Cfg<2,2,1,2,32,false>,0>',
    'S11': 'gemm_tn_f32_kernel<Cfg<2,2,1,1,32,false>,0>',
    'SPLITK': 'gemm_splitk_f32_kernel',
    'FEWROWS': 'gemm_fewrows_kernel',
}
WIDE_1 = 'gemm_wide_f32_kernel<1>'
LARGE_1 = 'gemm_tn_f32_kernel<Cfg<4,2,2,2,32,false>,1>'

# (kernel, variant, M, N, K, options).  variant: waves of the split-K kernel, rows of the few-rows kernel (the name does
# not tell them apart: `gemm_variant` mirrors launch_splitk / launch_fewrows), None otherwise.
LINEAR_CASES = [
    # the 256 x 256 tile: K tiles even / odd in number; a last K tile with only its first 4 columns, and with all but
    # its last 4
    ('WIDE', None, 7940, 2048, 64, {}),
    ('WIDE', None, 7940, 2048, 68, {}),
    ('WIDE', None, 7940, 2048, 92, {}),
    ('WIDE', None, 7940, 2048, 96, {}),
    ('WIDE', None, 7940, 2048, 100, {}),
    ('WIDE', None, 3841, 4096, 100, {}),
    ('LARGE', None, 1930, 4000, 100, {}),
    ('LARGE', None, 7940, 2048, 100, {'gemm_wide': 0}),
    ('S21', None, 130, 61, 100, {'gemm_splitk': 0}),
    ('S12', None, 61, 130, 44, {'gemm_splitk': 0}),
    ('S12', None, 2100, 1000, 72, {}),
    ('S11', None, 1, 4, 4, {}),
    ('S11', None, 40, 50, 36, {}),
    ('S11', None, 1000, 512, 144, {'gemm_splitk': 0}),
    ('SPLITK', 4, 33, 95, 68, {}),
    ('SPLITK', 4, 300, 1000, 1024, {}),
    ('SPLITK', 8, 100, 64, 1028, {}),
    ('SPLITK', 8, 257, 500, 1100, {}),
    # neighbours of the few-rows condition: one row too many, one column too few, four k past the LDS cap
    ('SPLITK', 8, 17, 67, 2048, {}),
    ('SPLITK', 8, 16, 63, 2048, {}),
    ('SPLITK', 8, 16, 64, 2052, {}),
    ('FEWROWS', 4, 3, 64, 1024, {}),
    ('FEWROWS', 8, 7, 130, 1100, {}),
    ('FEWROWS', 12, 12, 512, 2048, {}),
    ('FEWROWS', 16, 16, 67, 2048, {}),
    ('FEWROWS', 4, 2, 65, 2308, {}),      # K > 2048: a second pass over the weight row
]

# (id, scale, shift, act, slope, residual)
EPILOGUES = [
    ('none', False, False, 0, 0.0, False),
    ('scale_shift', True, True, 0, 0.0, False),
    ('shift_prelu_negative_slope', False, True, 1, -1.25, False),
    ('shift_prelu_positive_slope', False, True, 1, 0.25, False),
    ('prelu_residual', True, True, 1, 0.25, True),
    ('act2_residual', True, True, 2, 0.0, True),
    ('act2_no_residual', False, True, 2, 0.0, False),
]

PAD = 1e18          # behind the K columns of A and W: finite, so that a kernel may zero only one operand of a padded product
UNTOUCHED = -7.0    # pre-fill of C


def leading_dims(N, K):
    """lda, ldw, ldc, ldr: all larger than the logical width, all different (lda and ldw multiples of 4)."""
    return K + 8, K + 12, N + 3, N + 5


def pick_gemm(M, N, K, splitk=1, wide=1):
    """`pick_gemm` of csrc/gemm_f32.hip for one problem, mirrored (the GPU tests assert the library's own answer)."""
    cdiv = lambda a, b: (a + b - 1) // b
    nblocks = lambda bm, bn: cdiv(M, bm) * cdiv(N, bn)
    if splitk and M <= 16 and K >= 1024 and N >= 64 and ((M + 3) & ~3) * K * 4 <= 128 * 1024:
        return 'FEWROWS'
    if splitk and K >= 64 and nblocks(32, 32) <= 512:
        return 'SPLITK'
    narrow, shortm = N <= 64, M <= 64
    if shortm and narrow:
        return 'S11'
    if shortm:
        return 'S12'
    if narrow:
        return 'S21'
    if wide and N % 256 == 0 and K >= 64:
        t = nblocks(256, 256)
        if t >= 256 and t * 10 >= cdiv(t, 256) * 256 * 8:
            return 'WIDE'
    if nblocks(128, 128) >= 512:
        return 'LARGE'
    return 'S12' if nblocks(64, 128) >= 256 else 'S11'


def gemm_variant(kernel, M, N, K):
    """Waves of the split-K launch (launch_splitk) / row variant of the few-rows launch (launch_fewrows)."""
    if kernel == 'SPLITK':
        return 8 if K >= 1024 and ((M + 31) // 32) * ((N + 31) // 32) <= 256 else 4
    if kernel == 'FEWROWS':
        return (M + 3) // 4 * 4
    return None


def _set(**opts):
    lib = _lib.lib()
    for k, v in opts.items():
        _lib.check(lib.empose_set_option(k.encode(), int(v)))


def _kernel_name(M, N, K, count=1, role=0):
    return _lib.lib().empose_profile_gemm_kernel_name(M, N, K, count, role).decode()


def _padded(rows, cols, ld, g, fill=PAD, sd=1.0):
    t = torch.full((rows, ld), fill, device=DEV)
    t[:, :cols] = torch.randn(rows, cols, device=DEV, generator=g) * sd
    return t


def _report(reports):
    for r in reports:
        print(r.message.splitlines()[0])
    bad = [r.message for r in reports if not r.ok]
    assert not bad, '\n'.join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# a. Every kernel of launch_gemm, every epilogue form
@pytest.mark.parametrize('kernel,variant,M,N,K,opts', LINEAR_CASES,
                         ids=['%s%s-%dx%dx%d%s' % (c[0], '' if c[1] is None else c[1], c[2], c[3], c[4],
                                                   ''.join('-%s%d' % kv for kv in sorted(c[5].items())))
                              for c in LINEAR_CASES])
def test_linear_every_kernel_every_epilogue_every_element_within_its_allowance(kernel, variant, M, N, K, opts):
    lib = _lib.lib()
    _set(**opts)
    assert _kernel_name(M, N, K) == KERNEL_NAMES[kernel], 'pick_gemm no longer sends this shape to ' + kernel
    assert gemm_variant(kernel, M, N, K) == variant
    lda, ldw, ldc, ldr = leading_dims(N, K)
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + K)
    a = _padded(M, K, lda, g)
    w = _padded(N, K, ldw, g, sd=K ** -0.5)
    scale = (torch.rand(N, device=DEV, generator=g) + 0.5) * (1 - 2 * (torch.rand(N, device=DEV, generator=g) < 0.3).float())
    shift = torch.randn(N, device=DEV, generator=g)
    resid = _padded(M, N, ldr, g)
    products = E.gemm_products(a[:, :K], w[:, :K])
    c = torch.empty(M + 1, ldc, device=DEV)        # one guard row below M
    reports, untouched = [], []
    for eid, use_scale, use_shift, act, slope, use_resid in EPILOGUES:
        c.fill_(UNTOUCHED)
        _lib.check(lib.empose_linear_f32_ex(_lib.dptr(a), lda, _lib.dptr(w), ldw, _lib.dptr(c), ldc, M, N, K,
                                            _lib.dptr(scale) if use_scale else None, _lib.dptr(shift) if use_shift else None,
                                            _lib.dptr(resid) if use_resid else None, ldr if use_resid else 0, act, slope,
                                            _lib.current_stream()))
        torch.cuda.synchronize()
        want, allow = E.gemm_reference(None, None, scale if use_scale else None, shift if use_shift else None,
                                       resid[:, :N] if use_resid else None, act, slope, GAMMA, products=products)
        reports.append(E.check('%s %dx%dx%d %s' % (kernel, M, N, K, eid), c[:M, :N], want, allow, GAMMA))
        untouched.append((eid, bool((c[:M, N:] == UNTOUCHED).all()), bool((c[M] == UNTOUCHED).all())))
    _report(reports)
    for eid, pad_ok, guard_ok in untouched:
        assert pad_ok, '%s: columns [N, ldc) of C were written' % eid
        assert guard_ok, '%s: the row below M of C was written' % eid


# ----------------------------------------------------------------------------------------------------------------------
# b. Two problems per launch, ROLE 1: the layer-by-layer update MLPs
T_UPDATE = 16379      # 64 row tiles of 256 x 2 column tiles x 2 nets = 256 tiles of the 256 x 256 kernel; ragged last panel


def _update_net(skip):
    from em_pose_amd import synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    from tests import helpers as H
    from tests.test_hip_round5 import _randomize_bn
    torch.manual_seed(11)
    net = create_model(lgd_config(12, False, 1, m_skip_connections=skip), SMPLLayer(H.small_model()))
    _randomize_bn(net, 12)
    net.vertex_ids = synthetic.small_vertex_ids(160)
    return net.to(DEV).eval()


@pytest.fixture(scope='module')
def update_case():
    """The 512-wide nets of test_x3_elementwise._update_net, their input and their float64 references, computed once."""
    from tests.test_x3_elementwise import _update_net as plain_net
    xg = torch.randn(T_UPDATE, 296, generator=torch.Generator().manual_seed(T_UPDATE)).to(DEV)
    out = {}
    for skip in (False, True):
        net = _update_net(True) if skip else plain_net()
        sd = {k: v.detach() for k, v in net.state_dict().items() if not k.startswith('smpl.')}
        refs = [E.eval_mlp_reference(E.eval_mlp_layers(sd, p), xg, GAMMA, skip=skip)
                for p in ('pose_net_iter.', 'shape_net_iter.')]
        out[skip] = (net, refs)
    return xg, out


@pytest.mark.parametrize('skip', [False, True], ids=['plain', 'skip_connections'])
@pytest.mark.parametrize('wide', [1, 0], ids=['wide_tile', 'large_tile'])
def test_update_nets_layer_by_layer_two_problem_launches_within_their_allowance(update_case, wide, skip):
    from tests.test_x3_elementwise import _update_nets_fwd
    xg, nets = update_case
    net, refs = nets[skip]
    T = T_UPDATE
    _set(mlp_fused=0, gemm_wide=wide)
    # input layer (ROLE 0, ragged K), hidden layers (ROLE 1), the 66- / 10-column output layer as one launch
    assert _kernel_name(T, 512, 296, 2, 0) == (KERNEL_NAMES['WIDE'] if wide else KERNEL_NAMES['LARGE'])
    assert _kernel_name(T, 512, 512, 2, 1) == (WIDE_1 if wide else LARGE_1)
    assert _kernel_name(T, 66, 512, 2, 0) == KERNEL_NAMES['S12']
    outs = _update_nets_fwd(net, xg)
    torch.cuda.synchronize()
    _report([E.check('update nets layer by layer T=%d gemm_wide=%d skip=%d %s' % (T, wide, skip, name), got, want, allow,
                     GAMMA) for name, got, (want, allow) in zip(('pose', 'shape'), outs, refs)])


# ----------------------------------------------------------------------------------------------------------------------
# c. The strided split-K kernel of the small-problem training path
STRIDED_SHAPES = [(37, 45, 30), (100, 66, 297), (384, 512, 513), (33, 40, 44), (70, 31, 39)]   # K % 8 = 6, 1, 1, 4, 7
STRIDED_LAYOUTS = ['k_contiguous', 'gathered', 'k_contiguous_unaligned_base', 'k_contiguous_odd_row_stride']


def _strided_operand(rows, K, layout, g, sd=1.0):
    """(storage kept alive, pointer, row stride, k stride, the logical [rows][K] view)."""
    if layout == 'gathered':                       # stored [K][rows + 3]: the transposed matrix read as it lies
        st = _padded(K, rows, rows + 3, g, sd=sd)
        return st, st.data_ptr(), 1, rows + 3, st[:, :rows].t()
    if layout == 'k_contiguous_odd_row_stride':
        ld = K + 1 if (K + 1) % 4 else K + 2
        st = _padded(rows, K, ld, g, sd=sd)
        return st, st.data_ptr(), ld, 1, st[:, :K]
    ld = (K + 3) // 4 * 4 + 4
    if layout == 'k_contiguous':
        st = _padded(rows, K, ld, g, sd=sd)
        return st, st.data_ptr(), ld, 1, st[:, :K]
    flat = torch.full((rows * ld + 1,), PAD, device=DEV)      # the matrix starts one float into a 16-byte aligned buffer
    view = flat[1:].view(rows, ld)
    view[:, :K] = torch.randn(rows, K, device=DEV, generator=g) * sd
    return flat, flat.data_ptr() + 4, ld, 1, view[:, :K]


@pytest.mark.parametrize('M,N,K', STRIDED_SHAPES)
def test_gemm_strided_every_instantiation_every_element_within_its_allowance(M, N, K):
    lib = _lib.lib()
    assert lib.empose_gemm_strided_applicable(M, N) == 1
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    bias = torch.randn(N, device=DEV, generator=g)
    ldc = N + 3
    c = torch.empty(M + 1, ldc, device=DEV)
    reports, untouched = [], []
    for la in STRIDED_LAYOUTS:
        a_st, a_ptr, a_rs, a_ks, a = _strided_operand(M, K, la, g)
        for lw in STRIDED_LAYOUTS:
            w_st, w_ptr, w_rs, w_ks, w = _strided_operand(N, K, lw, g, sd=K ** -0.5)
            products = E.gemm_products(a, w)
            for use_bias in (True, False):
                c.fill_(UNTOUCHED)
                _lib.check(lib.empose_gemm_strided_f32(M, N, K, a_ptr, a_rs, a_ks, w_ptr, w_rs, w_ks, _lib.dptr(c), ldc,
                                                       _lib.dptr(bias) if use_bias else None, _lib.current_stream()))
                torch.cuda.synchronize()
                want, allow = E.gemm_reference(None, None, None, bias if use_bias else None, gamma=GAMMA, products=products)
                tag = 'strided %dx%dx%d A %s, W %s, bias %d' % (M, N, K, la, lw, use_bias)
                reports.append(E.check(tag, c[:M, :N], want, allow, GAMMA))
                untouched.append((tag, bool((c[:M, N:] == UNTOUCHED).all()) and bool((c[M] == UNTOUCHED).all())))
    worst = max(reports, key=lambda r: r.worst)
    print(worst.message.splitlines()[0])
    bad = [r.message for r in reports if not r.ok]
    assert not bad, '\n'.join(bad)
    for tag, ok in untouched:
        assert ok, tag + ': C was written outside its M x N elements'


# ----------------------------------------------------------------------------------------------------------------------
# d. C = A^T B and the column sums of A (weight and bias gradient of a linear layer)
ATB_SHAPES = [(384, 512, 512), (8192, 512, 296), (1000, 66, 512), (50, 10, 512), (4096, 2048, 144), (7, 5, 3),
              (130, 200, 320), (24576, 512, 512), (20000, 515, 500)]        # = test_hip_parity.py::test_gemm_atb_vs_float64


@pytest.mark.parametrize('aligned', [False, True], ids=['odd_leading_dims', 'aligned_leading_dims'])
@pytest.mark.parametrize('M,N,K', ATB_SHAPES)
def test_gemm_atb_every_element_within_its_allowance(M, N, K, aligned):
    """odd_leading_dims: the leading dimensions of the existing test (the general kernel); aligned: multiples of 4 (the
    LDS-staged kernels, and the interior kernel where the shape is whole tiles)."""
    lib = _lib.lib()
    lda, ldb, ldc = (N + 4 - N % 4 + 4, K + 4 - K % 4 + 8, K + 2) if aligned else (N + 3, K + 5, K + 2)
    g = torch.Generator(device=DEV).manual_seed(M + N)
    a, b = _padded(M, N, lda, g), _padded(M, K, ldb, g)
    a64, b64 = a[:, :N].double(), b[:, :K].double()
    want, allow = a64.t() @ b64, GAMMA * E.U * (a64.abs().t() @ b64.abs())
    want_b, allow_b = a64.sum(0), GAMMA * E.U * a64.abs().sum(0)
    c = torch.full((N + 1, ldc), UNTOUCHED, device=DEV)
    bias = torch.full((N + 1,), UNTOUCHED, device=DEV)
    nbytes = lib.empose_gemm_atb_workspace_bytes(M, N, K)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        _lib.check(lib.empose_gemm_atb_f32(M, N, K, _lib.dptr(a), lda, _lib.dptr(b), ldb, _lib.dptr(c), ldc,
                                           _lib.dptr(bias), _lib.dptr(ws), ws.numel(), _lib.current_stream()))
        torch.cuda.synchronize()
        runs.append((c.clone(), bias.clone()))
    _report([E.check('atb %dx%dx%d C' % (M, N, K), c[:N, :K], want, allow, GAMMA),
             E.check('atb %dx%dx%d column sums' % (M, N, K), bias[:N, None], want_b[:, None], allow_b[:, None], GAMMA)])
    assert bool((c[:N, K:] == UNTOUCHED).all()) and bool((c[N] == UNTOUCHED).all()) and float(bias[N]) == UNTOUCHED
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])     # bitwise reproducible
