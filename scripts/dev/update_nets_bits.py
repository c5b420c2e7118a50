"""Dev: do two builds of the library give the same bits from empose_update_nets_fwd?

  EMPOSE_LIB_PATH=<one build> python scripts/dev/update_nets_bits.py save a.pt
  EMPOSE_LIB_PATH=<other build> python scripts/dev/update_nets_bits.py save b.pt      (a process loads one library)
  python scripts/dev/update_nets_bits.py compare a.pt b.pt

The matrix: every form of the fused update MLPs (through the options), hidden widths 64 / 128 / 512 (every layer split by
K; the two widths that split columns over one and four waves), T = 8135 (the fewest rows of the one-launch path, ragged
last panel) and T = 16384 + 64 + 7.  Seeded weights and inputs; every output of every case must be torch.equal.
"""
import sys

import torch

FORMS = {'pair16': {}, 'x3_16': {'mlp_pair16': 0}, 'x3_32': {'mlp_fused16': 0}, 'fp32': {'mlp_x3': 0}}
HIDDEN = (64, 128, 512)
ROWS = (127 * 64 + 7, 16384 + 64 + 7)


def save(path):
    sys.path.insert(0, '.')
    from em_pose_amd import _lib, synthetic
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    dev = torch.device('cuda:0')
    lib = _lib.lib()
    body = SMPLLayer(synthetic.make_model())
    out = {}
    for hidden in HIDDEN:
        torch.manual_seed(100 + hidden)
        net = create_model(lgd_config(12, False, 1, hidden=hidden), body).to(dev).eval()
        h = net._ensure_handle(dev)
        for T in ROWS:
            x = torch.randn(T, 296, generator=torch.Generator().manual_seed(T + hidden)).to(dev)
            nb = lib.empose_update_workspace_bytes(h, T)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            for form, opts in FORMS.items():
                lib.empose_reset_options()
                for k, v in opts.items():
                    _lib.check(lib.empose_set_option(k.encode(), v))
                dp, ds = torch.full((T, 66), float('nan'), device=dev), torch.full((T, 10), float('nan'), device=dev)
                _lib.check(lib.empose_update_nets_fwd(h, T, _lib.dptr(x), 296, _lib.dptr(dp), _lib.dptr(ds), _lib.dptr(ws), nb, None))
                torch.cuda.synchronize()
                assert torch.isfinite(dp).all() and torch.isfinite(ds).all(), (form, hidden, T)
                out[(form, hidden, T)] = (dp.cpu(), ds.cpu())
    lib.empose_reset_options()
    torch.save(out, path)
    print('saved %d cases from %s' % (len(out), _lib.LIB_PATH))


def compare(a_path, b_path):
    a, b = torch.load(a_path, weights_only=False), torch.load(b_path, weights_only=False)
    assert a.keys() == b.keys()
    bad = 0
    for key in a:
        same = all(torch.equal(u, v) for u, v in zip(a[key], b[key]))
        differs_from_default = not all(torch.equal(u, v) for u, v in zip(a[key], a[('pair16',) + key[1:]]))
        print('form %-6s hidden %3d T %5d: %s%s' % (key + ('equal' if same else 'DIFFERENT',
                                                    '' if key[0] == 'pair16' or differs_from_default else '  (same bits as pair16?)')))
        bad += not same
    print('%d of %d cases differ' % (bad, len(a)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(save(sys.argv[2]) if sys.argv[1] == 'save' else compare(sys.argv[2], sys.argv[3]))
