#!/usr/bin/env python
"""
Converts a tree of AMASS `*.npz` sequences into the LMDB key schema the training reads (the AMASS half of reference
scripts/preprocess_amass_3dpw.py:23-60,126-189): every sequence resampled to 60 Hz on the GPU (data/resample.py, ragged
batches of one launch per kind), its 22 joints by forward kinematics of the resampled poses, then the seven records per
sequence plus `__len__` (data/datasets.py).

    python scripts/preprocess_amass.py --amass_dir DIR --out amass_lmdb --smpl_model model.npz

The records go into an LMDB environment when the `lmdb` package is importable; otherwise into `<out>.npz`, one array of
bytes per key, which `load_records` turns back into the dictionary `LMDBDataset(records)` accepts.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

DENYLIST = ('MTR03_poses.npz', 'WalkingStraightBackwards08_poses.npz')


def amass_file_ids(amass_dir):
    """The reference's file rules: every `*.npz` that is not a `*shape.npz` and not on the denylist, directories and files
    in sorted order; the id of a sequence is its path relative to `amass_dir`, with forward slashes."""
    ids = []
    for root, dirs, names in os.walk(amass_dir):
        dirs.sort()
        for f in sorted(names):
            if f.endswith('.npz') and not f.endswith('shape.npz') and f not in DENYLIST:
                ids.append(os.path.relpath(os.path.join(root, f), amass_dir).replace(os.sep, '/'))
    return ids


def convert_amass(amass_dir, smpl_model, fps=None, batch_size=64, device=None, put=None):
    """Resamples the tree in ragged batches of `batch_size` sequences and hands every record to `put(key, value)`;
    returns the records as a dictionary when `put` is None.  `smpl_model`: an `SMPLLayer` on the GPU."""
    import torch
    from em_pose_amd.data.data import AMASSSample
    from em_pose_amd.data.datasets import LMDB_LEN_KEY, encode_sequence_records
    from em_pose_amd.data.resample import resample_samples
    from em_pose_amd.helpers.configuration import CONSTANTS as C
    fps = float(C.FPS if fps is None else fps)
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    records = {} if put is None else None
    put = records.__setitem__ if put is None else put
    ids = amass_file_ids(amass_dir)
    for at in range(0, len(ids), batch_size):
        samples = []
        for file_id in ids[at:at + batch_size]:
            raw = np.load(os.path.join(amass_dir, file_id))
            gender = raw['gender'].tolist() if 'gender' in raw.files else 'unknown'
            samples.append(AMASSSample(file_id, raw['poses'][:, :C.MAX_INDEX_ROOT_AND_BODY], raw['betas'][:C.N_SHAPE_PARAMS],
                                       raw['trans'], raw['mocap_framerate'].tolist(),
                                       gender=gender.decode() if isinstance(gender, bytes) else str(gender)))
        resample_samples(samples, fps, device=device)
        # the joints of the whole batch in one forward-kinematics call, sequences at the target rate included
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
        poses = torch.cat([up(s.poses) for s in samples])
        betas = torch.cat([up(s.shape).reshape(1, -1).expand(s.n_frames, -1) for s in samples])
        trans = torch.cat([up(s.trans) for s in samples])
        joints = smpl_model.fk_joints(poses[:, 3:], betas, poses_root=poses[:, :3], trans=trans)
        joints = joints.reshape(poses.shape[0], -1).cpu().numpy()
        row = 0
        for k, s in enumerate(samples):
            rec = encode_sequence_records(at + k, s.id, s.poses, s.shape, s.trans, joints[row:row + s.n_frames], s.gender)
            row += s.n_frames
            for key, value in rec.items():
                put(key, value)
    put(LMDB_LEN_KEY, str(len(ids)).encode())
    return records


def save_records(path, records):
    """The records dictionary as one npz: keys as array names, values as uint8 arrays."""
    np.savez(path, **{k.decode(): np.frombuffer(v, dtype=np.uint8) for k, v in records.items()})


def load_records(path):
    """What `save_records` wrote, as the dictionary `LMDBDataset` accepts."""
    z = np.load(path)
    return {k.encode(): z[k].tobytes() for k in z.files}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--amass_dir', required=True)
    p.add_argument('--out', required=True, help='LMDB directory (with `lmdb`), else <out>.npz')
    p.add_argument('--smpl_model', default=None, help='SMPL-H model.npz (default: the synthetic stand-in body model)')
    p.add_argument('--fps', type=float, default=None, help='target rate (default 60)')
    p.add_argument('--batch_size', type=int, default=64, help='sequences per launch')
    args = p.parse_args()
    import torch
    from em_pose_amd import synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    if not torch.cuda.is_available():
        raise SystemExit('preprocess_amass.py runs the HIP path and needs an MI355X; there is no CPU fallback.')
    dev = torch.device('cuda', 0)
    smpl = SMPLLayer(args.smpl_model if args.smpl_model else synthetic.make_model()).to(dev)
    try:
        import lmdb
    except ImportError:
        lmdb = None
    if lmdb is None:
        out = args.out if args.out.endswith('.npz') else args.out + '.npz'
        save_records(out, convert_amass(args.amass_dir, smpl, args.fps, args.batch_size, dev))
        print('wrote', out)
        return
    env = lmdb.open(args.out, map_size=1 << 33)
    with env.begin(write=True) as txn:
        convert_amass(args.amass_dir, smpl, args.fps, args.batch_size, dev, put=txn.put)
    env.close()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
