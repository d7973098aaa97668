"""Loading the metric networks' weight files.  There is no surrogate: a missing file, key or shape raises RuntimeError naming them,
so that a number computed from anything but the real weights is never reported as FID or LPIPS."""
import os

import torch

INCEPTION_FILE = 'pt_inception-2015-12-05-6726825d.pth'    # metrics/pytorch_fid/inception.py
ALEXNET_FILE = 'alexnet-owt-7be5be79.pth'                  # torchvision models.alexnet(pretrained=True)
LPIPS_FILE = 'lpips_weights.ckpt'                          # metrics/lpips.py: 'metrics/lpips_weights.ckpt'


def hub_path(name):
    return os.path.join(torch.hub.get_dir(), 'checkpoints', name)


def resolve(weights, candidates, what):
    """(state dict, source name): `weights` as a state dict or a path, else the first existing file of `candidates`."""
    if isinstance(weights, dict):
        return _strip(weights), '<state dict>'
    paths = [weights] if weights else candidates
    for p in paths:
        if p and os.path.isfile(p):
            sd = torch.load(p, map_location='cpu')
            if not isinstance(sd, dict):
                raise RuntimeError('%s weights %s: not a state dict' % (what, p))
            return _strip(sd), p
    raise RuntimeError('%s weights not found (looked for %s). They are not shipped with hoig_amd; pass their path explicitly. '
                       'No metric is computed without them.' % (what, ', '.join(str(p) for p in paths)))


def _strip(sd):
    return {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in sd.items()}


def take(sd, source, key, shape):
    """sd[key] as fp64 on the host, checked against `shape`."""
    if key not in sd:
        raise RuntimeError('%s: missing key %s' % (source, key))
    t = sd[key]
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
        raise RuntimeError('%s: key %s has shape %s, expected %s' % (
            source, key, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, tuple(shape)))
    return t.detach().double().cpu()
