"""
Hand-written training step of the LGD models (BASELINE.json configs[4]).

The reference trains `IterativeErrorFeedback` through torch.autograd: `forward` builds a graph over the LSTM, the N
update-network applications and N + 1 body-model evaluations, `backward` sums the loss terms and calls
`total_loss.backward()` (reference nn/models.py:485-688).  The graph has a fixed, simple shape -- the update networks see
DETACHED inputs (models.py:549-551), so a parameter gradient only needs the cotangent of that application's output, and
estimates are chained by plain additions `pose_{i+1} = pose_i + step * delta_i` -- so this module runs the same
computation as an explicit forward sweep and an explicit reverse sweep over the library's own kernels, without autograd:

  forward   LSTM (empose_lstm_train_fwd) or init MLPs, heads, then per iteration: body model + residual gradient
            (empose_smpl_sensors_fwd_bwd, writing the gradient features straight into the network input rows), the two
            update MLPs in training mode (empose_mlp_train_fwd: GEMMs + train-mode BatchNorm/PReLU kernels), window mean of
            the shape update, additive update; every estimate goes into stacked history buffers.
  backward  all loss terms and their cotangents in one kernel (empose_lgd_losses), then for i = N .. 0: body-model
            vector-Jacobian product (empose_smpl_sensors_vjp), accumulation of the estimate's cotangent (including the
            reference's `E_i.backward()` deposit, models.py:576), update-MLP parameter gradients accumulated over the
            iterations (empose_mlp_train_bwd), finally the heads and back-propagation through time
            (empose_lstm_train_bwd).  Gradients are added to `param.grad` like autograd's AccumulateGrad.

Covers the released configurations (no skip connections, BatchNorm on, dropout 0, one window per forward); anything
else stays on the autograd path of nn/models.py.
"""
import collections
import contextlib
import ctypes as C

import torch

from em_pose_amd import _lib
from em_pose_amd.nn import layers as _layers

# row widths (floats) of the estimates and of what the body model makes of them
POSE, SHAPE, MARKERS, ORIS = 66, 10, 36, 108
POSE_PAD, SHAPE_PAD = 68, 12     # cotangent rows of the networks' outputs: padded to a multiple of 4 with zero columns
# a network input row is [x0 (d_in) | pose_i | shape_i | g_pose | g_shape]: where the gradient features start, past d_in
G_POSE_COL, G_SHAPE_COL = POSE + SHAPE, POSE + SHAPE + POSE


def _ptr(t):
    return None if t is None else t.data_ptr()


class _MlpView(object):
    """Device-pointer view of one MLP (reference layers.py:46-77) for empose_mlp_train_*."""

    always_transpose = False     # A/B (scripts/train.py --weight_t): transposed weight copies even where the backward reads W itself

    def __init__(self, mlp):
        self.mlp = mlp
        self.specs = mlp.dense_specs()
        self.n_layers = len(self.specs)
        self.in_dim, self.hidden = self.specs[0][0].in_features, self.specs[0][0].out_features
        self.out_dim = self.specs[-1][0].out_features
        self.weight_t = None
        self.weight_x3 = None     # pack_forward_x3(): three-piece bf16 copies of the hidden layers' weights (large batches)
        self.weight_t_x3 = None   # prepare_backward(): ... of their transposed copies
        self.save_layout = 0      # fix_layout(): how this step's forward lays out its saved activations

    def fix_layout(self, lib, M):
        """Pin the save-buffer layout of this step to what the library's options select NOW: the backward and weight-gradient
        calls then read the buffer the way the forward wrote it, whatever happens to the options in between."""
        self.save_layout = 0
        layout = lib.empose_mlp_train_save_layout(C.byref(self.params()), int(M))
        if layout <= 0:
            _lib.check(layout)
        self.save_layout = layout

    @staticmethod
    def supported(mlp):
        specs = mlp.dense_specs()
        if getattr(mlp, 'skip_connection', False) or not getattr(mlp, 'use_batch_norm', True):
            return False
        if len(specs) > _lib.MAX_DENSE or getattr(mlp.dropout, 'p', 0.0) > 0:
            return False
        h = specs[0][0].out_features
        for lin, bn, act in specs[:-1]:
            if bn is None or act is None or lin.out_features != h or act.weight.numel() != 1 or bn.momentum is None:
                return False
        return specs[0][0].in_features % 4 == 0 and h % 4 == 0

    def params(self):
        p = _lib.MlpParams()
        p.n_layers, p.in_dim, p.hidden, p.out_dim = self.n_layers, self.in_dim, self.hidden, self.out_dim
        for l, (lin, bn, act) in enumerate(self.specs):
            p.weight[l], p.bias[l] = lin.weight.data_ptr(), lin.bias.data_ptr()
            if bn is not None:
                p.bn_weight[l], p.bn_bias[l] = bn.weight.data_ptr(), bn.bias.data_ptr()
                if bn.track_running_stats and bn.running_mean is not None:
                    p.bn_running_mean[l], p.bn_running_var[l] = bn.running_mean.data_ptr(), bn.running_var.data_ptr()
                    p.bn_num_batches[l] = bn.num_batches_tracked.data_ptr()
                p.prelu[l] = act.weight.data_ptr()
                p.bn_eps, p.bn_momentum = float(bn.eps), float(bn.momentum)
        p.save_layout = self.save_layout
        for name in ('weight_t', 'weight_x3', 'weight_t_x3'):     # once per step (prepare_backward / pack_forward_x3)
            for l, t in enumerate(getattr(self, name) or ()):
                if t is not None:
                    getattr(p, name)[l] = t.data_ptr()
        return p

    X3_MIN_ROWS = 1024       # below, the library runs these layers on other kernels (one-launch layers, fp32 tiles)

    def wants_x3(self, lib, M):
        """Whether the hidden layers' products of M rows run on three bf16 pieces (and so need the packed weights)."""
        return M is not None and M >= _MlpView.X3_MIN_ROWS and self.hidden % 64 == 0 and \
            lib.empose_get_option(b'train_x3') != 0

    def _pack_x3(self, lib, stream, W, ld, n_rows, n_cols):
        nbytes = lib.empose_pack_weight_x3_bytes(int(n_rows), int(n_cols))
        out = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=W.device)
        _lib.check(lib.empose_pack_weight_x3(W.data_ptr(), int(ld), int(n_rows), int(n_cols), out.data_ptr(), stream))
        return out

    def pack_forward_x3(self, lib, stream, M):
        """Three-piece bf16 copies (fragment order) of the hidden layers' weights for the forward products of this step:
        once per step, like the transposed copies -- the weights do not change inside a step.  Large batches only."""
        self.weight_x3 = None
        if not self.wants_x3(lib, M):
            return
        self.weight_x3 = []
        for lin, bn, _ in self.specs:
            n_out, n_in = lin.weight.shape
            self.weight_x3.append(self._pack_x3(lib, stream, lin.weight, n_in, n_out, n_in) if bn is not None else None)

    def prepare_backward(self, lib, stream, M=None):
        """W^T of layers 1.. (what dX = dY . W needs on the K-contiguous GEMM): once per step instead of once per
        application of the network -- the weights do not change inside a step.  Not at all when the backward of M rows
        reads W itself (the one-launch layers of small batches)."""
        self.weight_t = None
        if M is not None and not _MlpView.always_transpose:
            uses = lib.empose_mlp_train_uses_weight_t(C.byref(self.params()), int(M))
            if uses < 0:
                _lib.check(uses)
            if uses == 0:
                return
        self.weight_t = [None]
        for lin, _, _ in self.specs[1:]:
            n_out, n_in = lin.weight.shape
            ld = (n_out + 3) & ~3
            alloc = torch.empty if ld == n_out else torch.zeros    # only padding columns need the zeros
            t = alloc(n_in, ld, dtype=torch.float32, device=lin.weight.device)
            _lib.check(lib.empose_transpose_f32(n_out, n_in, lin.weight.data_ptr(), n_in, t.data_ptr(), ld, stream))
            self.weight_t.append(t)
        # ... and their three-piece bf16 copies for dA = dY . W on the bf16 matrix cores (the product against W^T
        # [in][ld]: "N" = in features, "K" = ld = out features padded to a multiple of 4 with zero columns)
        self.weight_t_x3 = None
        if self.wants_x3(lib, M):
            self.weight_t_x3 = [None] + [self._pack_x3(lib, stream, t, t.shape[1], t.shape[0], t.shape[1])
                                         for t in self.weight_t[1:]]

    def parameter_list(self):
        return [t for lin, bn, act in self.specs
                for t in (lin.weight, lin.bias) + ((bn.weight, bn.bias, act.weight) if bn is not None else ())]

    def grads(self, tensors):
        g, ptrs = _lib.MlpGrads(), iter([t.data_ptr() for t in tensors])     # (in the order of parameter_list())
        for l, (lin, bn, act) in enumerate(self.specs):
            g.weight[l], g.bias[l] = next(ptrs), next(ptrs)
            if bn is not None:
                g.bn_weight[l], g.bn_bias[l], g.prelu[l] = next(ptrs), next(ptrs), next(ptrs)
        return g


def _lstm_params(rnn, input_size, grads=None):
    """LstmParams of an LSTM stack and, with `grads` (one tensor per weight), LstmGrads; also returns the weights."""
    weights = [w for unit in rnn._unit_params() for w in unit]
    return _layers.lstm_structs(weights, rnn.num_layers, input_size, rnn.hidden_size, grads) + (weights,)


MAIN = None      # a stream of the plan is MAIN or the index of a side stream (0, 1)
StreamPlan = collections.namedtuple('StreamPlan', 'fwd_split bwd_split pose_bwd shape_bwd pose_wgrad shape_wgrad '
                                                  'join_before_wgrad fork_before_wgrad')


def stream_plan(use_side, side_parts, deferred):
    """Which stream runs which update network in a training step, decided once (the table is in DESIGN.md, section 8).
    Without `use_side` (the step is too small for `two_streams`) everything is on MAIN; without `deferred` (the weight
    gradients are formed per application) the reverse sweep is.  fwd_split / bwd_split: the shape network on side 0, forked
    every iteration (and joined in the forward only), instead of one paired call on MAIN.  'bwd3' needs 'bwd'."""
    on = lambda part: bool(use_side) and part in side_parts
    bwd_split, side_w = bool(deferred) and on('bwd'), bool(deferred) and on('wgrad')
    third = bwd_split and 'bwd3' in side_parts
    return StreamPlan(on('fwd'), bwd_split, 1 if third else MAIN, 0 if bwd_split else MAIN,
                      (1 if third else 0) if side_w else MAIN, 0 if side_w else MAIN,
                      bool(use_side and deferred and not side_w), side_w and not third)


# what produced the initial estimate and what its backward reads: the LSTM + two linear heads, or the two init MLPs
_LstmStart = collections.namedtuple('_LstmStart', 'y c0 lstm_save')
_MlpStart = collections.namedtuple('_MlpStart', 'views params saves')


class _Step(object):
    """What a training step keeps between forward() and backward() and between their phases; all on the main stream's pool."""
    __slots__ = ('B', 'F', 'T', 'deferred', 'plan',              # windows, frames, rows = B * F; see _prepare
                 'x0', 'scale',                                  # packed input rows (T, d_in); per-frame residual weight
                 'lens32', 'masks', 'offset_r', 'offset_t',
                 'pose_hist', 'shape_hist', 'markers_hist', 'ori_hist', 'joints_hist',    # (N + 1, T, width) each
                 'X', 'views', 'params', 'saves',                # update networks: input rows (N, T, d_x), _MlpViews,
                 'smpl_h', 'start',                              # MlpParams, saves per iteration; _LstmStart / _MlpStart
                 'tmp10', 'dp', 'ws_smpl', 'nb_smpl',            # scratch of the forward sweep; below, the reverse sweep:
                 # cotangents, the update networks' gradients (tensors, MlpGrads), (x, save, stash) per deferred application
                 'd_pose', 'd_shape', 'd_mark', 'd_ori', 'd_joints', 'loss_vals', 'Dp', 'Ds', 'vp', 'vs', 'dpad', 'dspad',
                 'ws_vjp', 'nb_vjp', 'grads', 'gstructs', 'pend')

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields.pop(name, None))
        assert not fields, fields.keys()


class LgdTrainEngine(object):
    batched_wgrad = True   # dW / db of the update networks once over the N iterations (False: per iteration; A/B and tests)
    # The two update networks of an iteration are independent of each other, forward and backward, and neither their
    # backward nor their weight gradients feed the cotangent chain (the reference detaches the network inputs,
    # models.py:584): with `two_streams` the shape network runs on a side stream beside the pose network, and the
    # weight-gradient products of both (throughput-bound A^T B GEMMs) run there beside the heads' backward and the
    # back-propagation through time of the LSTM (a latency-bound chain of small launches) on the main stream.
    # Pays from a few thousand frames per step on (256 windows: 12.0 -> 10.5 ms); below that the step is a chain of short
    # launches and the cross-stream hand-offs cost more than the overlap gives (12 windows: 4.2 -> 4.9 ms).
    two_streams = True
    two_streams_min_frames = 2048
    # which uses of the side streams are on (A/B: scripts/train.py --streams; placements: stream_plan()): 'fwd' the shape
    # network's forward beside the pose network's; 'bwd' its backward; 'bwd3' the pose network's backward on a second side
    # stream, so that the main stream is only the cotangent chain, the heads and back-propagation through time; 'wgrad' the
    # weight-gradient products behind them.  Measured at 256 windows (frames/s): none 684 k, fwd 713 k, bwd 714 k,
    # wgrad 695 k, all 795-810 k.
    side_parts = ('fwd', 'bwd', 'bwd3', 'wgrad')

    def __init__(self, net):
        self.net = net
        self.step = None          # _Step of the forward() that backward() has not consumed yet
        self._side_streams = {}
        self._use_side = False
        self._held, self._forked = [], set()      # main-stream workspaces held; side streams forked and not yet joined

    # ---- the side stream ------------------------------------------------------------------------------------------
    def _side(self, k=0):
        st = self._side_streams.get(k)
        if st is None or st.device != self.dev:
            st = self._side_streams[k] = torch.cuda.Stream(device=self.dev)
        return st

    def _fork(self, k=0):
        """Side stream k continues from what the main stream has enqueued so far."""
        if self._use_side:
            self._side(k).wait_stream(torch.cuda.current_stream(self.dev))
            self._forked.add(k)

    def _join(self, k=0):
        """The main stream continues after what side stream k has enqueued so far.  Only a stream that was forked since its
        last join is waited for: under HIP-graph capture a wait on an event of a stream that never joined the capture is an
        isolation error, and a step whose options leave a stream unused must not touch it."""
        if self._use_side and k in self._forked:
            torch.cuda.current_stream(self.dev).wait_stream(self._side(k))
            self._forked.discard(k)
        if not self._forked:
            self._held = []       # nothing is running beside the main stream: its workspaces may go back to the allocator

    def _join_all(self):
        """Join every side stream that is still forked, in index order (and no other: see _join)."""
        for k in sorted(self._forked):
            self._join(k)
        self._held = []

    def _hold(self, t):
        """A main-stream workspace must not go back to the allocator between a fork and the next join: the block would be
        handed to the next main-pool allocation, and that tensor may be written by the side stream (which forked before
        the main-stream kernels that still use the workspace were enqueued)."""
        if self._use_side and self._forked:
            self._held.append(t)
        return t

    @contextlib.contextmanager
    def _on_side(self, k=0):
        """Launches (and transient allocations: workspaces, freed right after the launch, must belong to the stream that
        uses them) inside go to the side stream.  Long-lived tensors are allocated outside, on the main stream's pool,
        and freed only after a join."""
        if not self._use_side or k is MAIN:
            yield
            return
        main_raw = self.stream
        with torch.cuda.stream(self._side(k)):
            self.stream = _lib.current_stream()
            try:
                yield
            finally:
                self.stream = main_raw

    @staticmethod
    def supported(net):
        if net.skip_connections or getattr(net.config, 'm_dropout_hidden', 0.0) > 0 or getattr(net.config, 'm_dropout', 0.0) > 0:
            return False
        mlps = [net.pose_net_iter, net.shape_net_iter] + ([] if net.rnn_init else [net.pose_net_init, net.shape_net_init])
        if not all(_MlpView.supported(m) for m in mlps):
            return False
        if net.rnn_init and (net.rnn.is_bidirectional or net.rnn.num_layers > 4 or net.rnn.learn_init_state):
            return False
        return net.input_size % 4 == 0 and net.input_iter_size % 4 == 0

    # ---- small helpers over the C ABI -------------------------------------------------------------------------
    def _axpby(self, rows, cols, alpha, x, ldx, beta, y, ldy, out, ldo):
        _lib.check(self.lib.empose_axpby2d(rows, cols, alpha, x, ldx, beta, y, ldy, out, ldo, self.stream))

    def _call(self, where, fn, nbytes, *args):
        """check(fn(*args, workspace, nbytes, stream)) with the workspace allocated on the stream that uses it -- MAIN: the
        main stream's pool, held while a side stream is forked (_hold); k: side stream k's, inside _on_side."""
        with self._on_side(where):
            ws = self._hold(self.ws(nbytes)) if where is MAIN else self.ws(nbytes)
            _lib.check(fn(*args, ws.data_ptr(), nbytes, self.stream))

    def _mlp_fwd(self, p, x, ldx, out, ld_out, M, where=MAIN):
        lib, rp = self.lib, C.byref(p)
        save = self.new(lib.empose_mlp_train_save_floats(rp, M))
        self._call(where, lib.empose_mlp_train_fwd, lib.empose_mlp_train_workspace_bytes(rp, M),
                   rp, M, x, ldx, out, ld_out, save.data_ptr())
        _layers.BN_STATS_GENERATION[0] += 1
        return save

    def _mlp_fwd_pair(self, ps, x, ldx, outs, ld_outs, M):
        """Both update networks of an iteration in one call (empose_mlp_train_fwd_pair: at the reference's training batch
        every layer of both is one launch); returns their save buffers."""
        lib, r0, r1 = self.lib, C.byref(ps[0]), C.byref(ps[1])
        s0, s1 = [self.new(lib.empose_mlp_train_save_floats(r, M)) for r in (r0, r1)]
        self._call(MAIN, lib.empose_mlp_train_fwd_pair, lib.empose_mlp_train_pair_workspace_bytes(r0, r1, M),
                   r0, r1, M, x, ldx, outs[0], ld_outs[0], outs[1], ld_outs[1], s0.data_ptr(), s1.data_ptr())
        _layers.BN_STATS_GENERATION[0] += 2
        return s0, s1

    def _mlp_bwd_deferred_pair(self, ps, gs, x, ldx, d_outs, ld_douts, saves, accumulate, M, stashes):
        lib, r0, r1 = self.lib, C.byref(ps[0]), C.byref(ps[1])
        self._call(MAIN, lib.empose_mlp_train_bwd_deferred_pair, lib.empose_mlp_train_pair_workspace_bytes(r0, r1, M),
                   r0, r1, M, x, ldx, d_outs[0], ld_douts[0], d_outs[1], ld_douts[1], saves[0].data_ptr(),
                   saves[1].data_ptr(), C.byref(gs[0]), C.byref(gs[1]), int(accumulate), stashes[0].data_ptr(),
                   stashes[1].data_ptr())

    def _new_stash(self, p, M):
        """Stash of one deferred application + the address of its d_out slot (row stride (out_dim + 3) & ~3): the
        cotangent kernel writes the output cotangent there directly, so the deferred backward copies nothing."""
        stash = self.new(self.lib.empose_mlp_train_stash_floats(C.byref(p), M))
        return stash, stash.data_ptr() + 4 * M * (p.n_layers - 1) * p.hidden

    def _mlp_bwd(self, p, g, x, ldx, d_out, ld_dout, save, accumulate, M, stash=None, where=MAIN):
        """Backward of one application: dW / db into `g`, or (deferred) the layer cotangents kept in `stash` instead."""
        lib, rp = self.lib, C.byref(p)
        fn, tail = (lib.empose_mlp_train_bwd, ()) if stash is None else (lib.empose_mlp_train_bwd_deferred, (stash.data_ptr(),))
        self._call(where, fn, lib.empose_mlp_train_workspace_bytes(rp, M),
                   rp, M, x, ldx, d_out, ld_dout, save.data_ptr(), C.byref(g), int(accumulate), *tail)

    def _mlp_wgrad(self, p, g, pend, ldx, M, where=MAIN):
        """dW, db of one network over all its applications `pend` = [(x, save, stash)]: one A^T B product per layer
        (empose_mlp_train_wgrad)."""
        lib, rp, n = self.lib, C.byref(p), len(pend)
        xs, saves, stashes = [(C.c_void_p * n)(*col) for col in zip(*[(x, sv.data_ptr(), sh.data_ptr()) for x, sv, sh in pend])]
        self._call(where, lib.empose_mlp_train_wgrad, lib.empose_mlp_train_wgrad_workspace_bytes(rp, n, M),
                   rp, n, M, xs, ldx, saves, stashes, C.byref(g), 0)

    def ws(self, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=self.dev)

    # ---- where gradients go -------------------------------------------------------------------------------------
    @staticmethod
    def gradient_order(net):
        """The parameters in the order in which the reverse sweep finishes their gradients: update networks, then what
        produced the initial estimate (heads, LSTM last).  `helpers.distributed.GradientBuckets` lays its flat buckets
        out in this order so that the first buckets can be all-reduced while the rest is still being computed."""
        mlps = [net.pose_net_iter, net.shape_net_iter] + ([] if net.rnn_init else [net.pose_net_init, net.shape_net_init])
        order = [p for mlp in mlps for p in _MlpView(mlp).parameter_list()]
        if net.rnn_init:
            order += [net.pose_net_init.weight, net.pose_net_init.bias, net.shape_net_init.weight, net.shape_net_init.bias]
            order += [w for unit in net.rnn._unit_params() for w in unit]
        seen, out = set(), []
        for p in order:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                out.append(p)
        return out

    def _grad_like(self, p):
        """Where the kernels write p's gradient: p's slice of a persistent flat bucket when a gradient sink is attached
        and nothing has been accumulated into p.grad yet (then the slice simply BECOMES p.grad), else a fresh tensor."""
        sink = getattr(self.net, '_grad_sink', None)
        if sink is not None and p.grad is None and p.requires_grad:
            view = sink.view_of(p)
            if view is not None:
                return view
        return torch.empty_like(p)

    def _deposit(self, named, where=MAIN):
        """autograd's AccumulateGrad for a finished group of parameters, then tell the sink that they are final: in the
        context of the stream that formed the gradients."""
        sink = getattr(self.net, '_grad_sink', None)
        with self._on_side(where):
            for p_, g_ in named:
                if not p_.requires_grad:
                    continue
                if p_.grad is None:
                    p_.grad = g_
                elif p_.grad.data_ptr() != g_.data_ptr():
                    self._axpby(1, g_.numel(), 1.0, g_.data_ptr(), g_.numel(), 1.0, p_.grad.data_ptr(), g_.numel(),
                                p_.grad.data_ptr(), g_.numel())
                if sink is not None:
                    sink.stage(p_)

    def new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.dev)

    # ---- forward ------------------------------------------------------------------------------------------------
    def forward(self, batch_inputs):
        net, N = self.net, self.net.N
        st = self.step = self._prepare(batch_inputs)
        T, tmp10, shape0 = st.T, st.tmp10.data_ptr(), st.shape_hist[0].data_ptr()
        with torch.cuda.device(self.dev):
            st.smpl_h = net._ensure_smpl_handle(self.dev)
            st.start = self._lstm_start() if net.rnn_init else self._mlp_start()     # pose_0, and shape rows in tmp10
            if net.shape_avg:                                                        # shape_0: their window mean
                _lib.check(self.lib.empose_window_mean(T, st.F, SHAPE, tmp10, SHAPE, shape0, SHAPE, self.stream))
            else:
                self._axpby(T, SHAPE, 1.0, tmp10, SHAPE, 0.0, None, 0, shape0, SHAPE)
            (st.views, st.params), st.saves = self._views((net.pose_net_iter, net.shape_net_iter), T), []
            st.X, st.dp = self.new(max(N, 1), T, net.input_iter_size), self.new(T, POSE)
            st.nb_smpl = self.lib.empose_smpl_workspace_bytes(st.smpl_h, T)
            st.ws_smpl = self.ws(st.nb_smpl)
            for i in range(N + 1):
                self._iteration_fwd(i)
        st.tmp10 = st.dp = st.ws_smpl = None
        hist = {'pose': list(st.pose_hist), 'shape': list(st.shape_hist), 'joints': list(st.joints_hist),
                'markers': list(st.markers_hist), 'markers_ori': list(st.ori_hist)}
        out = {'pose': st.pose_hist[N].reshape(st.B, st.F, POSE), 'shape': st.shape_hist[N].reshape(st.B, st.F, SHAPE),
               'joints': st.joints_hist[N].reshape(st.B, st.F, POSE)}
        return out, hist

    def _prepare(self, batch_inputs):
        """Device and stream of the step, its packed inputs, its stream plan and its history buffers.  What lives until
        backward() is allocated here and in the phases on the MAIN stream's pool, never inside _on_side."""
        net = self.net
        if not batch_inputs['marker_pos'].is_cuda:
            raise _lib.EmposeError('IterativeErrorFeedback needs GPU tensors; there is no CPU fallback')
        dev = self.dev = batch_inputs['marker_pos'].device
        self.lib = _lib.lib()
        self.stream = _lib.current_stream()
        lens32 = batch_inputs['seq_lengths'].to(dev).to(torch.int32).contiguous()
        masks = batch_inputs['marker_masks'] if batch_inputs['marker_masks'] is None else \
            batch_inputs['marker_masks'].to(dev, torch.float32).contiguous()
        # network input rows + the per-frame weight of the in-loop residual (reference loss.py:36-39 times the B * F
        # rescale of models.py:578-579) in one launch
        from em_pose_amd.nn.models import pack_sensor_inputs
        inputs_, scale = pack_sensor_inputs(batch_inputs['marker_pos'], batch_inputs['marker_oris'], net.marker_idxs,
                                            masks, lens32, want_frame_weight=True)
        (B, F), n_hist = inputs_.shape[:2], net.N + 1
        T = B * F
        self._use_side = bool(self.two_streams and T >= self.two_streams_min_frames)
        deferred = self.batched_wgrad and 1 <= net.N <= 8   # (row counts off the 32-row grid: per application inside)
        return _Step(B=B, F=F, T=T, deferred=deferred, plan=stream_plan(self._use_side, self.side_parts, deferred),
                     x0=inputs_.reshape(T, net.input_size), scale=scale, lens32=lens32,
                     masks=None if masks is None else masks.reshape(T, 12),
                     offset_r=batch_inputs['offset_r'].to(dev, torch.float32).contiguous(),
                     offset_t=batch_inputs['offset_t'].to(dev, torch.float32).contiguous(),
                     pose_hist=self.new(n_hist, T, POSE), shape_hist=self.new(n_hist, T, SHAPE),
                     markers_hist=self.new(n_hist, T, MARKERS), ori_hist=self.new(n_hist, T, ORIS),
                     joints_hist=self.new(n_hist, T, POSE), tmp10=self.new(T, SHAPE))

    def _views(self, mlps, M):
        """_MlpViews of `mlps` with the save layout pinned and the x3 weights packed for M rows, and their MlpParams."""
        views = tuple(_MlpView(mlp) for mlp in mlps)
        for v in views:
            v.fix_layout(self.lib, M)
            v.pack_forward_x3(self.lib, self.stream, M)
        return views, [v.params() for v in views]

    def _lstm_start(self):
        """pose_0 and the shape rows (tmp10) from the LSTM over the input rows and the two linear heads."""
        net, lib, st, rnn = self.net, self.lib, self.step, self.net.rnn
        B, F, T, d_in, L, H = st.B, st.F, st.T, net.input_size, rnn.num_layers, rnn.hidden_size
        rnn.init_state = rnn.final_state
        p, _, _ = _lstm_params(rnn, d_in)
        h0, c0 = [t if t is None else t.detach().to(self.dev, torch.float32).contiguous() for t in rnn.init_state or (None, None)]
        y, h_n, c_n = self.new(T, H), self.new(L, B, H), self.new(L, B, H)
        save = self.new(lib.empose_lstm_train_save_floats(L, B, F, H))
        self._call(MAIN, lib.empose_lstm_train_fwd, lib.empose_lstm_train_workspace_bytes(C.byref(p), B, F),
                   C.byref(p), B, F, st.x0.data_ptr(), d_in, st.lens32.data_ptr(), _ptr(h0), _ptr(c0), y.data_ptr(),
                   h_n.data_ptr(), c_n.data_ptr(), save.data_ptr())
        rnn.final_state = (h_n, c_n)
        for lin, out, ld in ((net.pose_net_init, st.pose_hist[0], POSE), (net.shape_net_init, st.tmp10, SHAPE)):
            _lib.check(lib.empose_linear_f32(y.data_ptr(), H, lin.weight.data_ptr(), H, out.data_ptr(), ld, T,
                                             lin.out_features, H, None, lin.bias.data_ptr(), 0, 0.0, self.stream))
        return _LstmStart(y, c0, save)

    def _mlp_start(self):
        """pose_0 and the shape rows (tmp10) from the two init MLPs over the input rows."""
        st, d_in = self.step, self.net.input_size
        views, params = self._views((self.net.pose_net_init, self.net.shape_net_init), st.T)
        return _MlpStart(views, params, (
            self._mlp_fwd(params[0], st.x0.data_ptr(), d_in, st.pose_hist[0].data_ptr(), POSE, st.T),
            self._mlp_fwd(params[1], st.x0.data_ptr(), d_in, st.tmp10.data_ptr(), SHAPE, st.T)))

    def _iteration_fwd(self, i):
        """Body model (+ residual gradient) of estimate i and, for i < N, the two update networks and estimate i + 1."""
        net, lib, st = self.net, self.lib, self.step
        T, N, d_in, d_x = st.T, net.N, net.input_size, net.input_iter_size
        want_g = i < N and net.use_gradient
        Xi = st.X[i] if i < N else None
        _lib.check(lib.empose_smpl_sensors_fwd_bwd(
            st.smpl_h, T, st.F, st.pose_hist[i].data_ptr(), POSE, st.shape_hist[i].data_ptr(), SHAPE,
            st.offset_r.data_ptr(), st.offset_t.data_ptr(), st.x0.data_ptr() if want_g else None, d_in,
            st.scale.data_ptr() if want_g else None, st.markers_hist[i].data_ptr(), st.ori_hist[i].data_ptr(),
            st.joints_hist[i].data_ptr(), Xi[:, d_in + G_POSE_COL:].data_ptr() if want_g else None, d_x,
            Xi[:, d_in + G_SHAPE_COL:].data_ptr() if want_g else None, d_x, st.ws_smpl.data_ptr(), st.nb_smpl, self.stream))
        if i == N:
            return
        # network input rows [x0 | pose_i | shape_i | g_pose | g_shape] (the gradients are already there)
        _lib.check(lib.empose_lgd_assemble_inputs(T, d_in, st.x0.data_ptr(), d_in, st.pose_hist[i].data_ptr(),
                                                  st.shape_hist[i].data_ptr(), Xi.data_ptr(), d_x, self.stream))
        dp, ds = st.dp.data_ptr(), st.tmp10.data_ptr()
        if st.plan.fwd_split:                          # the two networks side by side
            self._fork(0)
            sp = self._mlp_fwd(st.params[0], Xi.data_ptr(), d_x, dp, POSE, T)
            ss = self._mlp_fwd(st.params[1], Xi.data_ptr(), d_x, ds, SHAPE, T, where=0)
            self._join(0)
        else:                                          # one stream: both networks per call (paired launches)
            sp, ss = self._mlp_fwd_pair(st.params, Xi.data_ptr(), d_x, (dp, ds), (POSE, SHAPE), T)
        st.saves.append((sp, ss))
        # pose_{i+1} = pose_i + s dp, shape_{i+1} = shape_i + s (window mean of) ds
        _lib.check(lib.empose_lgd_additive_update(
            st.B, st.F, float(net.step_size), int(bool(net.shape_avg)), st.pose_hist[i].data_ptr(), dp,
            st.shape_hist[i].data_ptr(), ds, st.pose_hist[i + 1].data_ptr(), st.shape_hist[i + 1].data_ptr(), self.stream))

    # ---- backward -----------------------------------------------------------------------------------------------
    def backward(self, batch, as_tensors=False):
        """Loss values + parameter gradients (added to `.grad`).  :return: (total loss tensor, loss_vals dict)"""
        if self.step is None:
            raise RuntimeError('backward() needs the preceding training-mode forward()')
        st, T = self.step, self.step.T
        with torch.cuda.device(self.dev):
            self.stream = _lib.current_stream()
            self._losses(batch)
            st.nb_vjp = self.lib.empose_smpl_vjp_workspace_bytes(st.smpl_h, T)
            st.ws_vjp = self.ws(st.nb_vjp)
            st.Dp, st.Ds, st.vp, st.vs = self.new(T, POSE), self.new(T, SHAPE), self.new(T, POSE), self.new(T, SHAPE)
            st.dpad, st.dspad = [torch.zeros(T, w, dtype=torch.float32, device=self.dev)   # zero padding columns for the GEMMs
                                 for w in (POSE_PAD, SHAPE_PAD)]
            st.grads = [[self._grad_like(p) for p in v.parameter_list()] for v in st.views]
            for v in st.views:
                v.prepare_backward(self.lib, self.stream, T)
            st.params = [v.params() for v in st.views]        # (with this step's weight_t / weight_t_x3)
            st.gstructs = [v.grads(g) for v, g in zip(st.views, st.grads)]
            st.pend = ([], [])
            for i in range(self.net.N, -1, -1):
                self._iteration_bwd(i)
            self._update_wgrads()
            self._start_bwd()
            self._join_all()
        self.step = None
        keys = ('pose', 'shape', 'reconstruction', 'fk', 'total_loss')
        host = st.loss_vals if as_tensors else st.loss_vals.tolist()
        return st.loss_vals[4], {k: host[j] for j, k in enumerate(keys)}

    def _losses(self, batch):
        """All loss terms and the cotangents of every history entry in one kernel (empose_lgd_losses)."""
        net, lib, st = self.net, self.lib, self.step
        B, F, T, n_hist = st.B, st.F, st.T, net.N + 1
        f32 = lambda t: t.to(self.dev, torch.float32).contiguous()
        io = _lib.LossIO()
        io.B, io.F, io.n_hist, io.n_markers = B, F, n_hist, net.n_markers
        io.marker_idx[:len(net.marker_idxs)] = [int(v) for v in net.marker_idxs]
        pose_gt, shape_gt = f32(batch.poses).reshape(T, POSE), f32(batch.shapes)
        joints_gt = f32(batch.joints_gt).reshape(T, POSE) if net.do_fk else None
        st.d_pose, st.d_shape, st.d_joints = self.new(n_hist, T, POSE), self.new(n_hist, T, SHAPE), self.new(T, POSE)
        st.d_mark, st.d_ori, st.loss_vals = self.new(n_hist, T, MARKERS), self.new(n_hist, T, ORIS), self.new(5)
        io.pose_hist, io.shape_hist, io.joints_final = [_ptr(t) for t in (st.pose_hist, st.shape_hist, st.joints_hist[net.N])]
        io.markers_hist, io.markers_ori_hist = st.markers_hist.data_ptr(), st.ori_hist.data_ptr()
        io.pose_gt, io.shape_gt, io.joints_gt = pose_gt.data_ptr(), shape_gt.data_ptr(), _ptr(joints_gt)
        io.inputs, io.ld_inputs, io.seq_lengths, io.marker_masks = st.x0.data_ptr(), net.input_size, _ptr(st.lens32), _ptr(st.masks)
        io.w_pose, io.w_shape, io.w_rec = float(net.pose_weight), float(net.shape_weight), float(net.r_weight)
        io.w_fk = float(net.fk_loss_weight) if net.do_fk else 0.0
        io.d_pose, io.d_shape, io.d_markers, io.d_markers_ori = [_ptr(t) for t in (st.d_pose, st.d_shape, st.d_mark, st.d_ori)]
        io.d_joints, io.loss_vals = st.d_joints.data_ptr(), st.loss_vals.data_ptr()
        self._call(MAIN, lib.empose_lgd_losses, lib.empose_lgd_losses_workspace_bytes(B, F, n_hist), C.byref(io))

    def _iteration_bwd(self, i):
        """Cotangent of estimate i and, for i > 0, the backward of the update networks' application that produced it."""
        net, lib, st = self.net, self.lib, self.step
        T, N, d_in, d_x, plan = st.T, net.N, net.input_size, net.input_iter_size, st.plan
        _lib.check(lib.empose_smpl_sensors_vjp(
            st.smpl_h, T, st.F, st.pose_hist[i].data_ptr(), POSE, st.shape_hist[i].data_ptr(), SHAPE,
            st.offset_r.data_ptr(), st.offset_t.data_ptr(), st.d_mark[i].data_ptr(), st.d_ori[i].data_ptr(),
            st.d_joints.data_ptr() if i == N else None, st.vp.data_ptr(), st.vs.data_ptr(), st.ws_vjp.data_ptr(), st.nb_vjp,
            self.stream))
        # running cotangents of the estimates (loss terms + body-model VJP + the reference's in-forward
        # `E_i.backward()` deposit, models.py:576: dE_i/d(pose_i) = g_i / (B F) flows into everything that produced
        # pose_i) and, for i > 0, the zero-padded cotangents of the update networks' outputs of iteration i - 1
        deposit = i < N and net.use_gradient
        dp_ptr, ds_ptr = st.dpad.data_ptr(), st.dspad.data_ptr()
        if st.deferred and i > 0:   # straight into the d_out slots of this application's stashes
            (stash_p, dp_ptr), (stash_s, ds_ptr) = self._new_stash(st.params[0], T), self._new_stash(st.params[1], T)
        _lib.check(lib.empose_lgd_cotangent_step(
            st.B, st.F, int(i == N), st.d_pose[i].data_ptr(), st.d_shape[i].data_ptr(), st.vp.data_ptr(),
            st.vs.data_ptr(), st.X[i][:, d_in + G_POSE_COL:].data_ptr() if deposit else None, d_x,
            st.X[i][:, d_in + G_SHAPE_COL:].data_ptr() if deposit else None, d_x, st.Dp.data_ptr(), st.Ds.data_ptr(),
            float(net.step_size), int(bool(net.shape_avg)), dp_ptr if i > 0 else None, ds_ptr if i > 0 else None, self.stream))
        if i == 0:
            return
        x, (sp, ss), acc, (p_p, p_s), (g_p, g_s) = st.X[i - 1].data_ptr(), st.saves[i - 1], i < N, st.params, st.gstructs
        if not st.deferred:
            self._mlp_bwd(p_p, g_p, x, d_x, dp_ptr, POSE_PAD, sp, acc, T)
            self._mlp_bwd(p_s, g_s, x, d_x, ds_ptr, SHAPE_PAD, ss, acc, T)
            return
        # weight gradients once over all N applications (one A^T B per layer instead of N).  Nothing below reads what
        # these calls write until the weight-gradient products: the backward of every iteration trails on its side
        # stream (shape network: side 0; pose network: main, or side 1 as the third stream), in order, without a join
        if plan.bwd_split:
            self._fork(plan.shape_bwd)
            if plan.pose_bwd is not MAIN:
                self._fork(plan.pose_bwd)
            self._mlp_bwd(p_p, g_p, x, d_x, dp_ptr, POSE_PAD, sp, acc, T, stash_p, where=plan.pose_bwd)
            self._mlp_bwd(p_s, g_s, x, d_x, ds_ptr, SHAPE_PAD, ss, acc, T, stash_s, where=plan.shape_bwd)
        else:                                          # one stream: both networks per call (paired launches)
            self._mlp_bwd_deferred_pair(st.params, st.gstructs, x, d_x, (dp_ptr, ds_ptr), (POSE_PAD, SHAPE_PAD),
                                        (sp, ss), acc, T, (stash_p, stash_s))
        st.pend[0].append((x, sp, stash_p))
        st.pend[1].append((x, ss, stash_s))

    def _update_wgrads(self):
        """Weight gradients of both update networks over all deferred applications where the plan puts them: on side streams
        they run beside the initial estimate's backward on the main stream (three streams: each network's products follow
        its own backward on its own stream, no fork needed).  Per-application gradients (`deferred` off) are only deposited."""
        st, plan = self.step, self.step.plan
        if plan.join_before_wgrad:       # (A/B: backward on side streams but the products on the main one)
            self._join_all()
        if plan.fork_before_wgrad:
            self._fork(0)
        for k, where in enumerate((plan.pose_wgrad, plan.shape_wgrad)):
            if st.pend[k]:
                self._mlp_wgrad(st.params[k], st.gstructs[k], st.pend[k], self.net.input_iter_size, st.T, where)
            if self.net.N > 0:   # final: a gradient sink may start averaging them while the rest of the sweep runs
                self._deposit(list(zip(st.views[k].parameter_list(), st.grads[k])), where)

    def _start_bwd(self):
        """Backward of what produced the initial estimate, from the zero-padded cotangents of pose_0 and shape_0."""
        net, st, T = self.net, self.step, self.step.T
        self._axpby(T, POSE, 1.0, st.Dp.data_ptr(), POSE, 0.0, None, 0, st.dpad.data_ptr(), POSE_PAD)
        Ds = st.Ds
        if net.shape_avg:
            Ds = self.new(T, SHAPE)
            _lib.check(self.lib.empose_window_mean(T, st.F, SHAPE, st.Ds.data_ptr(), SHAPE, Ds.data_ptr(), SHAPE, self.stream))
        self._axpby(T, SHAPE, 1.0, Ds.data_ptr(), SHAPE, 0.0, None, 0, st.dspad.data_ptr(), SHAPE_PAD)
        (self._lstm_start_bwd if isinstance(st.start, _LstmStart) else self._mlp_start_bwd)(st.start)

    def _lstm_start_bwd(self, start):
        """The two heads (weight gradients, cotangent of the LSTM output), then back-propagation through time."""
        net, lib, st, rnn = self.net, self.lib, self.step, self.net.rnn
        T, H, d_in = st.T, rnn.hidden_size, net.input_size
        dy, named = self.new(T, H), []
        for lin, dpd, ld, n_out in ((net.pose_net_init, st.dpad, POSE_PAD, POSE), (net.shape_net_init, st.dspad, SHAPE_PAD, SHAPE)):
            gw, gb = self._grad_like(lin.weight), self._grad_like(lin.bias)
            wsa = self.ws(lib.empose_gemm_atb_workspace_bytes(T, n_out, H))
            _lib.check(lib.empose_gemm_atb_f32(T, n_out, H, dpd.data_ptr(), ld, start.y.data_ptr(), H, gw.data_ptr(), H,
                                               gb.data_ptr(), wsa.data_ptr(), wsa.numel(), self.stream))
            wt = torch.zeros(H, ld, dtype=torch.float32, device=self.dev)
            _lib.check(lib.empose_transpose_f32(n_out, H, lin.weight.data_ptr(), H, wt.data_ptr(), ld, self.stream))
            _lib.check(lib.empose_linear_f32_ex(dpd.data_ptr(), ld, wt.data_ptr(), ld, dy.data_ptr(), H, T, H, ld,
                                                None, None, dy.data_ptr() if named else None, H, 0, 0.0, self.stream))
            named += [(lin.weight, gw), (lin.bias, gb)]
        self._deposit(named)
        lg = [self._grad_like(w) for unit in rnn._unit_params() for w in unit]
        p, g, weights = _lstm_params(rnn, d_in, lg)
        self._call(MAIN, lib.empose_lstm_train_bwd, lib.empose_lstm_train_workspace_bytes(C.byref(p), st.B, st.F),
                   C.byref(p), st.B, st.F, st.x0.data_ptr(), d_in, st.lens32.data_ptr(), _ptr(start.c0),
                   start.lstm_save.data_ptr(), dy.data_ptr(), None, C.byref(g))
        self._deposit(list(zip(weights, lg)))

    def _mlp_start_bwd(self, start):
        """The two init MLPs, weight gradients per network (one application each)."""
        st, named = self.step, []
        for v, p, sv, dpd, ld in zip(start.views, start.params, start.saves, (st.dpad, st.dspad), (POSE_PAD, SHAPE_PAD)):
            gi = [self._grad_like(p_) for p_ in v.parameter_list()]
            self._mlp_bwd(p, v.grads(gi), st.x0.data_ptr(), self.net.input_size, dpd.data_ptr(), ld, sv, False, st.T)
            named += list(zip(v.parameter_list(), gi))
        self._deposit(named)
