"""
The save-layout pin of the training MLPs (GPU; run with `-m gpu` on an MI355X).

A step's forward fixes how the save buffer is laid out (empose_mlp_params::save_layout, `_MlpView.fix_layout`); the reverse
sweep and the weight-gradient products of that step must read the buffer that way whatever the options say by then.
"""
import ctypes as C

import pytest
import torch

from em_pose_amd import _lib
from tests.test_hip_round5 import DEV, _mlp_pair, _run_mlp_train

pytestmark = pytest.mark.gpu

# forced layout: (its number, the options that select it, the options flipped to after the forward -- another layout)
LAYOUTS = {'passes': (1, {'train_fused': 0, 'train_epi': 0}, {'train_epi': 2}),
           'fused': (2, {'train_fused': 2}, {'train_fused': 0, 'train_epi': 0}),
           'epi': (3, {'train_epi': 2}, {'train_fused': 0, 'train_epi': 0})}
OPTIONS = ('train_cols', 'train_fused', 'train_epi')


def _set(lib, opts):
    for name, value in opts.items():
        _lib.check(lib.empose_set_option(name.encode(), value))


def _wgrad(res, x, M, accumulate=0, more=()):
    """dW, db of both networks from what the deferred sweep left (one application), through the views it was run with.
    `more`: further applications of the same networks, (their result, their x) each: one call over all of them;
    `accumulate`: added to the gradients in `res` instead of written."""
    lib = _lib.lib()
    for i, (view, save, stash, grads) in enumerate(zip(res['views'], res['save'], res['stash'], res['grads'])):
        p, g = view.params(), view.grads(grads)
        apps = [(x, save, stash)] + [(xk, rk['save'][i], rk['stash'][i]) for rk, xk in more]
        n = len(apps)
        arr = lambda k: (C.c_void_p * n)(*[_lib.dptr(app[k]) for app in apps])
        nbytes = lib.empose_mlp_train_wgrad_workspace_bytes(C.byref(p), n, M)
        ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=DEV)
        _lib.check(lib.empose_mlp_train_wgrad(C.byref(p), n, M, arr(0), x.shape[1], arr(1), arr(2), C.byref(g), accumulate,
                                              _lib.dptr(ws), nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    _lib.check(lib.empose_async_status())


def _flat(r):
    return list(r['out']) + list(r['save']) + list(r['stash']) + [t for gl in r['grads'] for t in gl] + \
        [t for b in r['bn'] for t in b]


@pytest.mark.parametrize('deferred', [True, False], ids=['deferred_wgrad', 'immediate'])
@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('M,in_dim,hidden', [(17, 152, 64), (48, 296, 32)])
def test_reverse_sweep_reads_the_layout_its_forward_wrote_whatever_the_options_say_then(M, in_dim, hidden, layout, deferred):
    """Forward under a forced layout, then the options flipped to select ANOTHER layout before the reverse sweep (deferred:
    and before empose_mlp_train_wgrad): the pinned parameters still report the forward's layout, and every output, saved
    record, stash, gradient and running statistic is bit-identical to the run whose options were left alone."""
    lib = _lib.lib()
    number, select, flip = LAYOUTS[layout]
    g = torch.Generator().manual_seed(M + hidden)
    x = torch.randn(M, in_dim, generator=g).to(DEV)
    d_outs = [torch.zeros(M, 68), torch.zeros(M, 12)]
    d_outs[0][:, :66] = torch.randn(M, 66, generator=g)
    d_outs[1][:, :10] = torch.randn(M, 10, generator=g)
    d_outs = [d.to(DEV) for d in d_outs]
    before = {name: lib.empose_get_option(name.encode()) for name in OPTIONS}
    res = {}
    try:
        for key in ('alone', 'flipped'):
            _set(lib, {'train_cols': 0})
            _set(lib, select)
            nets = _mlp_pair(in_dim, hidden, 5)
            hook = (lambda: _set(lib, flip)) if key == 'flipped' else None
            r = res[key] = _run_mlp_train(nets, x, d_outs, M, False, deferred, after_forward=hook)
            if deferred:
                _wgrad(r, x, M)
            for view in r['views']:
                p = view.params()
                assert p.save_layout == number
                assert lib.empose_mlp_train_save_layout(C.byref(p), M) == number
            if key == 'flipped':     # (the flip did select another layout for parameters that are not pinned)
                view.save_layout = 0
                p = view.params()
                assert lib.empose_mlp_train_save_layout(C.byref(p), M) not in (number, 0)
    finally:
        _set(lib, before)
    a, b = _flat(res['alone']), _flat(res['flipped'])
    assert len(a) == len(b)
    for want, got in zip(a, b):
        assert torch.isfinite(got.float()).all()
        assert torch.equal(want, got)
    # the weight gradients were formed, by the sweep itself or by empose_mlp_train_wgrad
    assert all(float(gl[0].abs().sum()) > 0.0 for gl in res['flipped']['grads'])
