"""
Resampling of motion sequences to another frame rate on the GPU (reference scripts/preprocess_amass_3dpw.py:63-123:
`resample_rotations` = SQUAD on the joint rotations, `resample_positions` = a not-a-knot cubic spline), through
`empose_resample_rotations` / `empose_resample_positions` (csrc/resample.hip).  One launch takes a ragged batch of
sequences.  Tensors live on the GPU; CPU tensors raise `_lib.EmposeError`, there is no fallback.

The translation side equals `scipy.interpolate.CubicSpline`.  The rotation side follows Shoemake's SQUAD with this
project's own treatment of the first and last segment: the reference takes SQUAD from the
`numpy-quaternion` package, against which the ends are not verified.
"""
import numpy as np
import torch

from em_pose_amd import _lib

# empose_resample_seq (include/empose_hip.h)
SEQ_DTYPE = np.dtype([('in_row', np.int32), ('f_in', np.int32), ('out_row', np.int32), ('f_out', np.int32),
                      ('fps_in', np.float64), ('fps_out', np.float64)])
assert SEQ_DTYPE.itemsize == 32


def n_frames_out(n_frames, fps_in, fps_out):
    """Number of output frames, by the reference's own arithmetic: `len(np.arange(0, duration, 1 / fps_out))`."""
    return len(np.arange(0, n_frames / fps_in, 1 / fps_out))


def sequence_table(lengths, fps_in, fps_out):
    """The host table of a packed ragged batch: sequence s reads `lengths[s]` rows after those of the sequences before it
    and writes `n_frames_out` rows likewise.  `fps_in` is one rate or one per sequence."""
    lengths = [int(n) for n in lengths]
    rates = np.broadcast_to(np.asarray(fps_in, dtype=np.float64), (len(lengths),))
    table = np.zeros(len(lengths), dtype=SEQ_DTYPE)
    table['f_in'] = lengths
    table['fps_in'], table['fps_out'] = rates, float(fps_out)
    table['f_out'] = [n_frames_out(n, r, float(fps_out)) for n, r in zip(lengths, rates)]
    table['in_row'] = np.cumsum([0] + lengths[:-1])
    table['out_row'] = np.cumsum([0] + table['f_out'][:-1].tolist())
    return table


def _table_ptr(table):
    assert table.dtype == SEQ_DTYPE and table.flags['C_CONTIGUOUS']
    return table.ctypes.data_as(_lib.C.c_void_p)


def _rows_checked(rows, what, n, table):
    """What can be refused before anything is copied to the GPU; the library checks the whole table again."""
    if not torch.is_tensor(rows) or not rows.is_cuda:
        raise _lib.EmposeError('{} must be a tensor on the GPU; there is no CPU fallback'.format(what))
    if n <= 0:
        raise _lib.EmposeError('{}: the number of joints or channels must be positive'.format(what))
    if len(table) == 0 or int(table['f_in'].min()) < 2:
        raise _lib.EmposeError('{}: resampling needs at least two frames per sequence'.format(what))
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise _lib.EmposeError('{} must be a contiguous float32 matrix of rows'.format(what))
    return rows


def resample_rotation_rows(rows, n_joints, table, out_ld=None):
    """empose_resample_rotations on `rows` (R, ld) float32 on the GPU, whose first 3 * n_joints columns are rotation
    vectors, for the sequences of `table` (SEQ_DTYPE): the packed output rows (sum of f_out, out_ld or 3 * n_joints);
    columns past the rotations are left unwritten."""
    rows = _rows_checked(rows, 'rotations', n_joints, table)
    out_rows = int(table['f_out'].sum())
    out_ld = 3 * n_joints if out_ld is None else out_ld
    with torch.cuda.device(rows.device):
        dev_table = torch.from_numpy(table.view(np.uint8)).to(rows.device)
        out = torch.empty(out_rows, max(out_ld, 0), dtype=torch.float32, device=rows.device)
        _lib.check(_lib.lib().empose_resample_rotations(len(table), _table_ptr(table), _lib.dptr(dev_table), n_joints,
                                                        _lib.dptr(rows), rows.shape[1], rows.shape[0], _lib.dptr(out),
                                                        out_ld, out_rows, _lib.current_stream()))
    return out


def resample_position_rows(rows, n_channels, table, out_ld=None):
    """empose_resample_positions on `rows` (R, ld) float32 on the GPU, whose first n_channels columns are resampled."""
    rows = _rows_checked(rows, 'positions', n_channels, table)
    out_rows = int(table['f_out'].sum())
    out_ld = n_channels if out_ld is None else out_ld
    lib = _lib.lib()
    with torch.cuda.device(rows.device):
        dev_table = torch.from_numpy(table.view(np.uint8)).to(rows.device)
        out = torch.empty(out_rows, max(out_ld, 0), dtype=torch.float32, device=rows.device)
        ws_bytes = lib.empose_resample_positions_workspace_bytes(rows.shape[0], n_channels)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=rows.device)
        _lib.check(lib.empose_resample_positions(len(table), _table_ptr(table), _lib.dptr(dev_table), n_channels,
                                                 _lib.dptr(rows), rows.shape[1], rows.shape[0], _lib.dptr(out), out_ld,
                                                 out_rows, _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return out


def _batched(sequences, fps_in, fps_out, rows_fn, per_item):
    """One launch for a list of (F_s, ...) tensors that agree in their trailing shape."""
    sequences = list(sequences)
    if not sequences:
        return []
    for x in sequences:
        if not torch.is_tensor(x) or not x.is_cuda:
            raise _lib.EmposeError('resampling needs tensors on the GPU; there is no CPU fallback')
    tail = tuple(sequences[0].shape[1:])
    if any(tuple(x.shape[1:]) != tail for x in sequences):
        raise ValueError('the sequences of a batch must agree in every dimension but the first')
    rates = np.broadcast_to(np.asarray(fps_in, dtype=np.float64), (len(sequences),))
    todo = [s for s in range(len(sequences)) if rates[s] != float(fps_out)]   # equal rates: the input, unchanged
    out = list(sequences)
    if todo:
        width = int(np.prod(tail, dtype=np.int64))
        if per_item == 3 and (not tail or tail[-1] != 3):
            raise _lib.EmposeError('rotations are (F, N, 3) rotation vectors')
        table = sequence_table([sequences[s].shape[0] for s in todo], rates[todo], fps_out)
        rows = torch.cat([sequences[s].reshape(sequences[s].shape[0], width).float() for s in todo], dim=0).contiguous()
        res = rows_fn(rows, width // per_item, table)
        for s, q in zip(todo, table):
            piece = res[int(q['out_row']):int(q['out_row']) + int(q['f_out'])]
            out[s] = piece.reshape((piece.shape[0],) + tail).to(sequences[s].dtype)
    return out


def resample_rotations_batch(sequences, fps_in, fps_out):
    """A list of (F_s, N, 3) rotation-vector sequences (GPU tensors; `fps_in` one rate or one per sequence) -> the list of
    (F'_s, N, 3) resampled sequences, in one launch."""
    return _batched(sequences, fps_in, fps_out, resample_rotation_rows, 3)


def resample_positions_batch(sequences, fps_in, fps_out):
    """A list of (F_s, ...) position sequences -> the list of (F'_s, ...) resampled sequences, in one launch."""
    return _batched(sequences, fps_in, fps_out, resample_position_rows, 1)


def resample_rotations(rotations, fps_in, fps_out):
    """(F, N, 3) rotation vectors at `fps_in` -> (F', N, 3) at `fps_out` (reference resample_rotations)."""
    return resample_rotations_batch([rotations], fps_in, fps_out)[0]


def resample_positions(positions, fps_in, fps_out):
    """(F, ...) positions at `fps_in` -> (F', ...) at `fps_out` (reference resample_positions)."""
    return resample_positions_batch([positions], fps_in, fps_out)[0]


def resample_samples(samples, fps_out, smpl_model=None, device=None):
    """Resamples `AMASSSample`s in place to `fps_out` with one launch per kind (rotations, translations): poses[:, :66] as
    22 rotations, trans, `fps`; `joints`, where a sample has them, are recomputed by forward kinematics of the resampled
    poses (`smpl_model.fk_joints`, the joints-only entry point), never interpolated.  Samples already at `fps_out` pass
    through untouched.  Host arrays go to `device` (default: the current GPU) and come back as float32 arrays; tensors stay
    tensors on their device."""
    from em_pose_amd.helpers.configuration import CONSTANTS as C
    n_pose = C.MAX_INDEX_ROOT_AND_BODY
    todo = [s for s in samples if float(s.fps) != float(fps_out)]
    if not todo:
        return samples
    if any(s.joints is not None for s in todo) and smpl_model is None:
        raise ValueError('samples with joints need the body model: the joints are recomputed, not interpolated')
    if device is None:
        gpu = [s.poses.device for s in todo if torch.is_tensor(s.poses) and s.poses.is_cuda]
        device = gpu[0] if gpu else torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
    up = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))) \
        .to(device=device, dtype=torch.float32)
    rates = [float(s.fps) for s in todo]
    poses = resample_rotations_batch([up(s.poses)[:, :n_pose].reshape(s.poses.shape[0], n_pose // 3, 3) for s in todo],
                                     rates, fps_out)
    trans = resample_positions_batch([up(s.trans) for s in todo], rates, fps_out)
    for s, p, t in zip(todo, poses, trans):
        p = p.reshape(p.shape[0], n_pose)
        joints = None
        if s.joints is not None:
            betas = up(s.shape).reshape(1, -1)
            joints = smpl_model.fk_joints(p[:, 3:], betas, poses_root=p[:, :3], trans=t).reshape(p.shape[0], -1)
        back = (lambda x, like: x.to(like.device, like.dtype)) if torch.is_tensor(s.poses) else \
            (lambda x, like: x.cpu().numpy())
        s.poses, s.trans = back(p, s.poses), back(t, s.trans)
        if joints is not None:
            s.joints = back(joints, s.joints)
        s.fps = torch.scalar_tensor(float(fps_out)).to(s.fps.dtype) if torch.is_tensor(s.fps) else float(fps_out)
    return samples
