"""
Generates tests/golden/normalize_root.npz by running the UNMODIFIED reference: the root normalisation of
`empose/bodymodels/smpl.py:112-119` through `empose.helpers.so3`, and `SMPLLayer._fk(normalize_root=True)` on the small
body model of tests/golden/smpl_small.npz.  Run from the repository root, with the reference checkout given:

    python tests/golden/make_golden_normalize_root.py <path of the reference checkout>

Nothing from the reference is copied: the script imports `empose.*` (third-party modules the image lacks come from
oracle/refstubs, as for make_golden.py: the body-model arithmetic is the oracle's), feeds it seeded inputs and stores
inputs and outputs.  Two sequences, of 40 frames and of 1 frame (groups `a/` and `b/`):

  poses_root, poses_body, betas, trans   float32 inputs; the relative root angles of `a` are spread over [0, 2.6] rad (the
                                         reference's acos-based logarithm loses accuracy toward pi and is no yardstick there)
  root32, trans32                        lines 112-119 in float32, as the reference's layer computes them
  root64, trans64                        the same lines, same functions, on the float32 inputs cast to float64
  err_root, err_trans                    max |32 - 64|: the reference's own fp32 error, the bar of the forward tests
  joints, vertices                       the reference layer's output (float32); `a` only
  error                                  the exception the reference layer raised, or ''

For N = 1 the `.squeeze()` of line 118 collapses trans to shape (3,), and line 119 then subtracts its FIRST COMPONENT from
all three (`trans[0:1]` of a vector): (0, ty - tx, tz - tx) of the rotated translation.  `b/trans32` records exactly that,
shape (3,), and the body model then refuses the shape (`b/error`), so the reference returns nothing for one frame.
`b/trans64` is what the lines mean, zeros of shape (1, 3), which is what this repository computes, shape (N, 3) kept.
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('EMPOSE_REFERENCE', '')
if not os.path.isdir(os.path.join(REF, 'empose')):
    raise SystemExit(__doc__)

_tmp = tempfile.mkdtemp(prefix='empose_golden_')
for k in ('EM_DATA_SYNTH', 'EM_EXPERIMENTS', 'SMPL_MODELS', 'EM_DATA_REAL'):
    os.environ[k] = _tmp
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'refstubs'))
sys.path.insert(0, REF)

import torch  # noqa: E402

from em_pose_amd.data.transforms import matrix_to_rotvec  # noqa: E402  (input generation only)
from em_pose_amd.eval.metrics import rotvec_to_matrix  # noqa: E402

torch.set_num_threads(4)


def inputs(rng, n, max_rel):
    root0 = rng.normal(0, 0.8, size=3)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.linspace(0.0, max_rel, n)
    rng.shuffle(ang[1:])
    ang[0] = 0.0
    R = rotvec_to_matrix(root0)[None] @ rotvec_to_matrix(axis * ang[:, None])
    root = matrix_to_rotvec(R)
    root[0] = root0
    return {'poses_root': root.astype(np.float32),
            'poses_body': rng.normal(0, 0.4, size=(n, 63)).astype(np.float32),
            'betas': rng.normal(0, 1, size=(n, 10)).astype(np.float32),
            'trans': rng.normal(0, 1, size=(n, 3)).astype(np.float32)}


class _Captured(Exception):
    pass


def normalised_by_reference(smpl, w, dtype, evaluate):
    """What `SMPLLayer._fk(normalize_root=True)` hands to its body model (root_orient, trans) -- lines 112-119 as the
    reference runs them, for inputs of `dtype` -- and, with `evaluate`, what the layer returns.  Without `evaluate` the
    call is cut off in front of the body model (whose buffers are float32)."""
    seen = {}

    def hook(module, args, kwargs):
        seen['root'], seen['trans'] = kwargs['root_orient'].detach().clone(), kwargs['trans'].detach().clone()
        if not evaluate:
            raise _Captured()
    t = {k: torch.from_numpy(v).to(dtype) for k, v in w.items()}
    handle = smpl.bm.register_forward_pre_hook(hook, with_kwargs=True)
    result, error = None, ''
    try:
        with torch.no_grad():
            result = smpl._fk(t['poses_body'], t['betas'], t['poses_root'], t['trans'], normalize_root=True)
    except _Captured:
        pass
    except Exception as e:   # the body model's own complaint (N = 1, see the module docstring)
        error = '{}: {}'.format(type(e).__name__, e)
    finally:
        handle.remove()
    return seen['root'], seen['trans'], result, error


def main():
    from empose.bodymodels.smpl import create_default_smpl_model
    d = os.path.join(_tmp, 'smplh_amass', 'neutral')
    os.makedirs(d, exist_ok=True)
    small = np.load(os.path.join(HERE, 'smpl_small.npz'))
    np.savez(os.path.join(d, 'model.npz'), **{k: small[k] for k in small.files})
    smpl = create_default_smpl_model(torch.device('cpu'))
    rng = np.random.default_rng(20240112)
    out = {}
    for tag, n in (('a', 40), ('b', 1)):
        w = inputs(rng, n, 2.6)
        root32, trans32, result, error = normalised_by_reference(smpl, w, torch.float32, True)
        root64, trans64, _, _ = normalised_by_reference(smpl, w, torch.float64, False)
        if n == 1:
            trans64 = torch.zeros(1, 3, dtype=torch.float64)
        for k, v in w.items():
            out['{}/{}'.format(tag, k)] = v
        out[tag + '/root32'], out[tag + '/trans32'] = root32.numpy(), trans32.numpy()
        out[tag + '/root64'], out[tag + '/trans64'] = root64.numpy(), trans64.numpy()
        out[tag + '/err_root'] = np.float64(np.abs(root32.double().numpy() - root64.numpy()).max())
        if n > 1:
            out[tag + '/err_trans'] = np.float64(np.abs(trans32.double().numpy() - trans64.numpy()).max())
        if result is not None:
            out[tag + '/vertices'], out[tag + '/joints'] = result[0].numpy(), result[1].numpy()
        out[tag + '/error'] = np.array(error)
        print(tag, n, 'err_root', float(out[tag + '/err_root']), 'err_trans', float(out.get(tag + '/err_trans', 0)), 'trans32', tuple(trans32.shape), 'error', error)
    np.savez_compressed(os.path.join(HERE, 'normalize_root.npz'), **out)


if __name__ == '__main__':
    main()
