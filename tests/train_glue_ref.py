"""Float64 restatements of the loss and bookkeeping kernels of the training step (csrc/train_loss.hip, csrc/train_glue.hip: lgd_losses,
lgd_cotangent_step, lgd_additive_update, lgd_assemble_inputs, window_mean, axpby2d), the per-element allowances they are
held to, input generators and thin callers of the C entry points.  Shared by tests/test_train_glue.py (GPU) and
tests/test_train_glue_bounds.py (CPU).  Not a test module; imports without a GPU.

Allowances.  The library is built without fast-math, so `/` and sqrtf are correctly rounded; FMA contraction is allowed, so
an output is compared with float64, never bitwise with an fp32 restatement (pure copies excepted).  Every output element
gets  chain * u * magnitude,  u = 2^-24:  `magnitude` is the same operation on absolute values (float64) and `chain` the
longest sequence of fp32 roundings between the inputs and that element, counted from the kernel source:

  CHAIN_SIGN = 5       pose / shape cotangents +-k, k = w * inv_n1 * inv / 66:  inv_n1 = 1 / N1 (1), the product (1),
                       inv = 1 / (len * B) (the product of two small integers is exact; the division 1), the product (1),
                       / 66 (1).
  CHAIN_UNIT = 14      sensor cotangents k r_c / |r|:  r = hat - gt (1);  |r|^2 is a sum of nine squares, each carrying
                       2 (r twice) + 1 (product) and up to 8 additions = 11, halved by the square root and one for sqrtf =
                       6.5;  k = w_rec * inv_n1 * inv (4);  k * r_c (1);  the division (1):  1 + 6.5 + 4 + 1 + 1 = 13.5.
                       Joints: three squares (5 -> 3.5), k = w_fk * inv (2): 8.5.  Both are within the cap of 32.
  CHAIN_RUN = 4        Dp / Ds / dpad / dspad without the window mean:  d + D (1), vp + . (1), inv_T * g + . (inv_T 1,
                       product 1, sum 1 -- the g term sees three, like the others), step * . (1).
  chain_mean(F) = F + 3    dspad under shape_avg, the figure the issue of these tests sets:  the three of Ds, the window
                       sum (the first addition to 0 is exact: F - 1), / F (1), step * . (1).  Counted rounding by rounding
                       the first two summands of a window pass F + 4 when the deposit is not contracted into an FMA,
                       summand f only F + 5 - f, and at F = 1 sum and quotient are exact (4 = F + 3): the figure stays as
                       stated, and a kernel that needs more is a finding, not a reason to raise it.
                       empose_window_mean alone: F - 1 additions and the division = F.
  chain_next(F) = 2 (F + 3)   shape_next under shape_avg (mean F, step * . 1, + shape 1 = F + 2 <= 2 (F + 3));
                       pose_next and shape_next without the mean: CHAIN_NEXT = 2.
  CHAIN_AXPBY = 3      alpha x (1), beta y (1), the sum (1).
  Loss values: the per-frame term is an fp32 chain, the sum over frames and history entries is double (2^-53, nothing
  beside u), the final cast to float one more:
    LOSS_CHAINS pose 70:   hat - gt (1), 65 additions, / 66 (1), * inv (1) with inv (1), the cast (1).
                shape 14:  1 + 9 + 1 + 1 + 1 + 1.
                reconstruction 26:  the orientation norm 6.5 as above, * inv (2), + the position term (1), the sum over the
                           16 lanes (4 levels), the cast (1) = 14.5 <= 26.
                fk 70:     a joint's norm 3.5, 21 additions, * inv (2), the cast (1) = 27.5 <= 70.
    total: sum_k w_k * (allowance of term k); the weights are fp32 values and the combination is double.
"""
import ctypes as C

import numpy as np
import torch

from oracle import torch_ref as R

U = 2.0 ** -24
CHAIN_SIGN, CHAIN_UNIT, CHAIN_RUN, CHAIN_NEXT, CHAIN_AXPBY = 5, 14, 4, 2, 3
CHAIN_CAP = 32          # the first three must stay below it
LOSS_CHAINS = (70, 14, 26, 70)   # pose, shape, reconstruction, fk
LOSS_NAMES = ('pose', 'shape', 'reconstruction', 'fk', 'total_loss')
COTANGENTS = ('d_pose', 'd_shape', 'd_markers', 'd_markers_ori', 'd_joints')
assert max(CHAIN_SIGN, CHAIN_UNIT, CHAIN_RUN) <= CHAIN_CAP


def chain_mean(F):
    return F + 3


def chain_next(F):
    return 2 * (F + 3)


def f32(x):
    """The value the kernel receives for a float argument."""
    return float(np.float32(x))


# ---- the losses and their cotangents ---------------------------------------------------------------------------------
def losses_torch(io, dtype=torch.float64):
    """The loss of IterativeErrorFeedback.backward and the cotangents of the total loss with respect to every history
    entry: torch autograd in `dtype` through the oracle's loss pieces, combined as reference models.py:648-680 (the FK
    term once per history entry, the total divided by n_hist).  `io`: dict with the fields of empose_loss_io as CPU
    tensors (`marker_idx` a list, `seq_lengths` / `marker_masks` / `joints_gt` may be None).
    :return: dict: 'loss_vals' (5,) pose, shape, reconstruction, fk, total_loss, and the five cotangent arrays."""
    B, F, N1, nm = io['B'], io['F'], io['n_hist'], io['n_markers']
    T = B * F
    t = lambda k: io[k].detach().cpu().to(dtype)
    lens = torch.full((B,), F, dtype=torch.int64) if io['seq_lengths'] is None else io['seq_lengths'].cpu().long()
    masks = None if io['marker_masks'] is None else t('marker_masks').reshape(B, F, 12)
    idx = [int(v) for v in list(io['marker_idx'])[:nm]]
    x = t('inputs')[:, :12 * nm].reshape(B, F, 12 * nm)
    pos_in, ori_in = x[..., :3 * nm].reshape(B, F, nm, 3), x[..., 3 * nm:].reshape(B, F, nm, 9)
    leaf = lambda k: t(k).clone().requires_grad_(True)
    ph, sh, mh, oh, jf = leaf('pose_hist'), leaf('shape_hist'), leaf('markers_hist'), leaf('markers_ori_hist'), \
        leaf('joints_final')
    pose_gt = t('pose_gt').reshape(B, F, 66)
    shape_gt = t('shape_gt').unsqueeze(1).repeat(1, F, 1)
    joints_gt = None if io['joints_gt'] is None else t('joints_gt').reshape(B, F, 22, 3)
    pose, shape, rec, fk = (torch.zeros((), dtype=dtype) for _ in range(4))
    for i in range(N1):
        pose = pose + R.padded_l1(pose_gt, ph[i].reshape(B, F, 66), lens)
        shape = shape + R.padded_l1(shape_gt, sh[i].reshape(B, F, 10), lens)
        if joints_gt is not None:
            fk = fk + R.reconstruction_loss(joints_gt, jf.reshape(B, F, 22, 3), lens, masks)
        rec = rec + R.reconstruction_loss(pos_in, mh[i].reshape(B, F, 12, 3)[:, :, idx], lens, masks)
        rec = rec + R.reconstruction_loss(ori_in, oh[i].reshape(B, F, 12, 9)[:, :, idx], lens, masks)
    w_pose, w_shape, w_fk, w_rec = (f32(io[k]) for k in ('w_pose', 'w_shape', 'w_fk', 'w_rec'))
    total = (w_pose * pose + w_fk * fk + w_shape * shape + w_rec * rec) / N1
    total.backward()
    g = lambda a: torch.zeros_like(a) if a.grad is None else a.grad
    return {'loss_vals': torch.stack([pose / N1, shape / N1, rec / N1, fk / N1, total]).detach(),
            'd_pose': g(ph), 'd_shape': g(sh), 'd_markers': g(mh), 'd_markers_ori': g(oh), 'd_joints': g(jf)}


def losses64(io):
    return losses_torch(io, torch.float64)


def losses_allowance(io, want):
    """Allowances of every output of `losses64`.  The loss terms are sums of non-negative numbers and a cotangent is a
    single product / quotient: the magnitude of each is its own absolute value (of the total: the weighted terms)."""
    lv = want['loss_vals'].abs()
    a = torch.stack([LOSS_CHAINS[k] * U * lv[k] for k in range(4)])
    w = torch.tensor([abs(f32(io[k])) for k in ('w_pose', 'w_shape', 'w_rec', 'w_fk')], dtype=torch.float64)
    out = {'loss_vals': torch.cat([a, (w * a).sum().reshape(1)])}
    for k in ('d_pose', 'd_shape'):
        out[k] = CHAIN_SIGN * U * want[k].abs()
    for k in ('d_markers', 'd_markers_ori', 'd_joints'):
        out[k] = CHAIN_UNIT * U * want[k].abs()
    return out


def dead_rows(io):
    """(padding, dropped): (T,) bool -- frames at or past their window's length; frames with a missing sensor."""
    B, F = io['B'], io['F']
    lens = torch.full((B,), F, dtype=torch.int64) if io['seq_lengths'] is None else io['seq_lengths'].cpu().long()
    padding = ~R.mask_from_seq_lengths(lens, F).reshape(-1)
    dropped = torch.zeros(B * F, dtype=torch.bool) if io['marker_masks'] is None else \
        ~(io['marker_masks'].cpu() != 0).all(dim=-1).reshape(-1)
    return padding, dropped


def make_loss_case(B, F, n_hist, n_markers, marker_idx, ld_extra=0, lengths=None, masks=None, fk=None, seed=0):
    """A loss problem whose residual norms are bounded away from zero (hat = gt + d, |d| >= 1e-3 per sensor and joint,
    asserted) and whose L1 terms contain entries with hat == gt exactly.
    lengths: None or 'ragged' (a window of length F, one of length 1 when B > 1); masks: None, 'ones' or 'zeros' (10 % of
    the entries zero, one window with every frame dropped and, where the model reads fewer than 12 sensors, a frame whose
    only missing sensor is one it does not read); fk: None (no joints_gt) or the weight."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + F + n_hist)
    T = B * F
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)

    def offset(*shape):          # a residual of norm 2e-3 .. 0.5 along the last axis
        d = rn(*shape)
        d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-6)
        return d * (2e-3 + 0.5 * torch.rand(*shape[:-1], 1, generator=g))
    idx = [int(v) for v in marker_idx][:n_markers]
    ld = 12 * n_markers + ld_extra
    inputs = rn(T, ld)
    pose_gt, shape_gt, joints_gt = 0.5 * rn(T, 66), rn(B, 10), rn(T, 66)
    pose_hist = pose_gt[None] + 0.3 * rn(n_hist, T, 66)
    shape_hist = shape_gt[None, :, None, :].expand(n_hist, B, F, 10).reshape(n_hist, T, 10) + 0.3 * rn(n_hist, T, 10)
    same = torch.rand(n_hist, T, 66, generator=g) < 0.05
    pose_hist = torch.where(same, pose_gt[None].expand_as(pose_hist), pose_hist)
    same = torch.rand(n_hist, T, 10, generator=g) < 0.1
    shape_hist = torch.where(same, shape_gt[None, :, None, :].expand(n_hist, B, F, 10).reshape(n_hist, T, 10), shape_hist)
    markers_hist, ori_hist = rn(n_hist, T, 12, 3), rn(n_hist, T, 12, 9)
    for slot, m in enumerate(idx):
        markers_hist[:, :, m] = inputs[None, :, 3 * slot:3 * slot + 3] + offset(n_hist, T, 3)
        ori_hist[:, :, m] = inputs[None, :, 3 * n_markers + 9 * slot:3 * n_markers + 9 * slot + 9] + offset(n_hist, T, 9)
        assert float((markers_hist[:, :, m] - inputs[None, :, 3 * slot:3 * slot + 3]).norm(dim=-1).min()) >= 1e-3
        assert float((ori_hist[:, :, m] - inputs[None, :, 3 * n_markers + 9 * slot:3 * n_markers + 9 * slot + 9])
                     .norm(dim=-1).min()) >= 1e-3
    joints_final = (joints_gt.reshape(T, 22, 3) + offset(T, 22, 3)).reshape(T, 66)
    assert float((joints_final - joints_gt).reshape(T, 22, 3).norm(dim=-1).min()) >= 1e-3
    seq_lengths = None
    if lengths == 'ragged':
        seq_lengths = torch.randint(1, F + 1, (B,), generator=g, dtype=torch.int32)
        seq_lengths[0] = F
        if B > 1:
            seq_lengths[1] = 1
    m = None
    if masks == 'ones':
        m = torch.ones(T, 12)
    elif masks == 'zeros':
        m = (torch.rand(B, F, 12, generator=g) >= 0.1).float()
        unread = [s for s in range(12) if s not in idx]
        if B * F == 1:
            m[:] = 1.0                                          # (a single frame: both properties at once)
        m[B - 1, :, unread[0] if unread else 5] = 0.0          # a window with every frame dropped
        if B > 1 or F > 1:
            m[0, 0] = 1.0                                       # a frame that counts
        if unread and (B > 1 or F > 1):
            m[0, F - 1] = 1.0                                   # the only missing sensor is one the model does not read
            m[0, F - 1, unread[-1]] = 0.0
        m = m.reshape(T, 12)
        assert not (m.reshape(B, F, 12)[B - 1] != 0).all(-1).any()
        if unread:
            lone = (m[:, idx] != 0).all(-1) & ~(m != 0).all(-1)
            assert lone.any()
    return {'B': B, 'F': F, 'n_hist': n_hist, 'n_markers': n_markers, 'marker_idx': idx,
            'pose_hist': pose_hist.contiguous(), 'shape_hist': shape_hist.contiguous(),
            'markers_hist': markers_hist.reshape(n_hist, T, 36).contiguous(),
            'markers_ori_hist': ori_hist.reshape(n_hist, T, 108).contiguous(), 'joints_final': joints_final,
            'pose_gt': pose_gt, 'shape_gt': shape_gt, 'joints_gt': None if fk is None else joints_gt,
            'inputs': inputs, 'seq_lengths': seq_lengths, 'marker_masks': m,
            'w_pose': 10.0, 'w_shape': 1.0, 'w_fk': 0.0 if fk is None else fk, 'w_rec': 0.01}


# ---- the bookkeeping kernels -----------------------------------------------------------------------------------------
def _window_mean(x, F):
    return x.reshape(-1, F, x.shape[-1]).mean(dim=1, keepdim=True).expand(-1, F, -1).reshape(x.shape)


def window_mean64(x, F):
    """out[t] = mean of x over the window of frame t (F consecutive rows)."""
    return _window_mean(x.detach().double(), F)


def window_mean_magnitude(x, F):
    return _window_mean(x.detach().double().abs(), F)


def additive_update64(B, F, step, shape_avg, pose, d_pose, shape, d_shape, magnitude=False):
    """pose_next = pose + step d_pose, shape_next = shape + step (mean over the window of) d_shape."""
    c = (lambda a: a.detach().double().abs()) if magnitude else (lambda a: a.detach().double())
    s = abs(f32(step)) if magnitude else f32(step)
    ds = c(d_shape)
    if shape_avg:
        ds = _window_mean(ds, F)
    return c(pose) + s * c(d_pose), c(shape) + s * ds


def cotangent_step64(B, F, first, d_pose, d_shape, vp, vs, g_theta, g_beta, Dp, Ds, step, shape_avg, magnitude=False):
    """Dp = [Dp +] d_pose + vp [+ g_theta / (B F)], Ds likewise; dpad = step Dp, dspad = step (window mean of) Ds.
    :return: (Dp, Ds, dpad (T,66), dspad (T,10)); with `magnitude` the same operations on absolute values."""
    c = (lambda a: a.detach().double().abs()) if magnitude else (lambda a: a.detach().double())
    s = abs(f32(step)) if magnitude else f32(step)
    inv_T = 1.0 / (B * F)
    new_p, new_s = c(d_pose) + c(vp), c(d_shape) + c(vs)
    if not first:
        new_p, new_s = new_p + c(Dp), new_s + c(Ds)
    if g_theta is not None:
        new_p = new_p + inv_T * c(g_theta)
    if g_beta is not None:
        new_s = new_s + inv_T * c(g_beta)
    return new_p, new_s, s * new_p, s * (_window_mean(new_s, F) if shape_avg else new_s)


def axpby64(alpha, x, beta, y, like, magnitude=False):
    """alpha x + beta y; x or y None = 0."""
    c = (lambda a: a.detach().double().abs()) if magnitude else (lambda a: a.detach().double())
    a, b = (abs(f32(alpha)), abs(f32(beta))) if magnitude else (f32(alpha), f32(beta))
    out = torch.zeros(like.shape, dtype=torch.float64)
    if x is not None:
        out = out + a * c(x)
    if y is not None:
        out = out + b * c(y)
    return out


def assemble64(x0, pose, shape):
    """X[t] = [x0[t] | pose[t] | shape[t]] (a pure copy: exact in any precision)."""
    return torch.cat([x0, pose, shape], dim=1)


# ---- the C entry points ----------------------------------------------------------------------------------------------
def nan_like(shape, dev):
    return torch.full(tuple(shape), float('nan'), dtype=torch.float32, device=dev)


def loss_io_struct(io, dev, keep):
    """empose_loss_io of a case on `dev`; every output buffer pre-filled with NaN.  `keep` receives the device tensors
    (inputs and outputs, by field name) so that they outlive the asynchronous call."""
    from em_pose_amd import _lib
    B, F, N1 = io['B'], io['F'], io['n_hist']
    T = B * F
    s = _lib.LossIO()
    s.B, s.F, s.n_hist, s.n_markers = B, F, N1, io['n_markers']
    for k, v in enumerate(io['marker_idx']):
        s.marker_idx[k] = int(v)
    for k in ('pose_hist', 'shape_hist', 'markers_hist', 'markers_ori_hist', 'joints_final', 'pose_gt', 'shape_gt',
              'joints_gt', 'inputs', 'marker_masks'):
        keep[k] = None if io[k] is None else io[k].to(dev, torch.float32).contiguous()
        setattr(s, k, None if keep[k] is None else keep[k].data_ptr())
    keep['seq_lengths'] = None if io['seq_lengths'] is None else io['seq_lengths'].to(dev, torch.int32).contiguous()
    s.seq_lengths = None if keep['seq_lengths'] is None else keep['seq_lengths'].data_ptr()
    s.ld_inputs = io['inputs'].shape[1]
    s.w_pose, s.w_shape, s.w_fk, s.w_rec = io['w_pose'], io['w_shape'], io['w_fk'], io['w_rec']
    for k, shape in (('d_pose', (N1, T, 66)), ('d_shape', (N1, T, 10)), ('d_markers', (N1, T, 36)),
                     ('d_markers_ori', (N1, T, 108)), ('d_joints', (T, 66)), ('loss_vals', (5,))):
        keep[k] = nan_like(shape, dev)
        setattr(s, k, keep[k].data_ptr())
    return s


def run_losses(io, dev='cuda:0'):
    """empose_lgd_losses on a case of CPU tensors -> dict of CPU float32 outputs ('loss_vals' + the five cotangents)."""
    from em_pose_amd import _lib
    lib = _lib.lib()
    keep = {}
    s = loss_io_struct(io, dev, keep)
    nbytes = lib.empose_lgd_losses_workspace_bytes(io['B'], io['F'], io['n_hist'])
    assert nbytes == 4 * io['n_hist'] * io['B'] * io['F'] * 4 + 256
    ws = torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.empose_lgd_losses(C.byref(s), _lib.dptr(ws), C.c_size_t(nbytes), _lib.current_stream()))
        torch.cuda.synchronize()
    return {k: keep[k].cpu() for k in ('loss_vals',) + COTANGENTS}


def run_cotangent_step(B, F, first, d_pose, d_shape, vp, vs, g_theta, ld_g, g_beta, ld_gb, Dp, Ds, step, shape_avg,
                       dpad, dspad):
    """Device tensors as the engine passes them (g_theta / g_beta may be views into a wider row block; Dp / Ds / dpad /
    dspad are updated in place)."""
    from em_pose_amd import _lib
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    return _lib.lib().empose_lgd_cotangent_step(B, F, int(first), p(d_pose), p(d_shape), p(vp), p(vs), p(g_theta), ld_g,
                                                p(g_beta), ld_gb, p(Dp), p(Ds), step, int(shape_avg), p(dpad), p(dspad),
                                                _lib.current_stream())


def run_additive_update(B, F, step, shape_avg, pose, d_pose, shape, d_shape):
    """-> (pose_next, shape_next), pre-filled with NaN."""
    from em_pose_amd import _lib
    pose_next, shape_next = nan_like(pose.shape, pose.device), nan_like(shape.shape, pose.device)
    _lib.check(_lib.lib().empose_lgd_additive_update(B, F, step, int(shape_avg), _lib.dptr(pose), _lib.dptr(d_pose),
                                                     _lib.dptr(shape), _lib.dptr(d_shape), _lib.dptr(pose_next),
                                                     _lib.dptr(shape_next), _lib.current_stream()))
    return pose_next, shape_next


def run_window_mean(T, F, Cc, x, out):
    from em_pose_amd import _lib
    _lib.check(_lib.lib().empose_window_mean(T, F, Cc, _lib.dptr(x), x.shape[1], _lib.dptr(out), out.shape[1],
                                             _lib.current_stream()))


def run_axpby(rows, cols, alpha, x, beta, y, out):
    """x / y / out: 2-D device tensors at least `cols` wide (their widths are the row strides) or None."""
    from em_pose_amd import _lib
    p = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    _lib.check(_lib.lib().empose_axpby2d(rows, cols, alpha, p(x), 0 if x is None else x.shape[1], beta, p(y),
                                         0 if y is None else y.shape[1], p(out), out.shape[1], _lib.current_stream()))


def run_assemble(T, d_in, x0, pose, shape, X):
    from em_pose_amd import _lib
    _lib.check(_lib.lib().empose_lgd_assemble_inputs(T, d_in, _lib.dptr(x0), x0.shape[1], _lib.dptr(pose),
                                                     _lib.dptr(shape), _lib.dptr(X), X.shape[1], _lib.current_stream()))
