"""The contract between PyTorch and the HIP kernels, once: a network's parameters are views into ONE flat fp32 buffer in
`parameters()` order (weight, then bias, module by module); the kernels, Adam and the all-reduce work on that buffer.  Here live
the slice table of such a layout, the views into a buffer, the binding of a module tree to it, the packed-weight cache of the MFMA
kernels (`FlatNet`, the base of model.NeRF and nerfpp.MLPNet), the `module.` prefix of the reference's checkpoints and the
exchange of the flat Adam moments with torch.optim.Adam."""
import math

import torch
from torch import nn

from . import ops


def slices(shapes):
    """[(module_name, (out, in))] -> ([(parameter_name, offset, shape)], total floats)."""
    out, off = [], 0
    for name, (o, i) in shapes:
        out.append((name + '.weight', off, (o, i)))
        off += o * i
        out.append((name + '.bias', off, (o,)))
        off += o
    return out, off


def views(flat, table):
    """{name: view of `flat`} for a slice table (the first result of slices())."""
    return {name: flat[off:off + math.prod(shape)].view(shape) for name, off, shape in table}


def bind(module, table, flat, flat_grad):
    """Move the parameters of a freshly constructed module tree into `flat` (their values are copied in) and make every
    parameter a view of it, with `.grad` the matching view of `flat_grad`."""
    mods = dict(module.named_modules())
    grads = views(flat_grad, table)
    for name, view in views(flat, table).items():
        mod_name, leaf = name.rsplit('.', 1)
        with torch.no_grad():
            view.copy_(getattr(mods[mod_name], leaf).detach().to(flat.device))
        p = nn.Parameter(view)
        p.grad = grads[name]
        setattr(mods[mod_name], leaf, p)


class FlatNet(nn.Module):
    """A network the MLP kernels run: `flat` (what they read, layout `kind` of include/fastnerf.h) and its packed copies."""
    kind = 0
    _packed = None

    def _sync_kernel_net(self):
        """Called before every re-pack: make `flat` current.  Nothing to do where `flat` IS the parameters; a network whose
        `flat` is derived from them (NeRF without view directions) overrides it."""

    def packed(self, refresh=True):
        """(packed_fwd, packed_bwd) fragment-ordered copies of the weights.  Re-packed from the
        flat buffer on every call unless refresh=False (one ~5 MB launch; callers that update
        the weights themselves, e.g. the fused Trainer, pass refresh=False between updates)."""
        if self._packed is None or self._packed_mode != ops.get_math():
            self._packed = (torch.empty(ops.packed_floats(self.kind, 1), device=self.flat.device),
                            torch.empty(ops.packed_floats(self.kind, 2), device=self.flat.device))
            self._packed_mode = ops.get_math()
            refresh = True
        if refresh:
            self._sync_kernel_net()
            ops.mlp_pack(self.flat, *self._packed, kind=self.kind)
        return self._packed


# ---- the nn.DataParallel prefix of the reference's checkpoints ---------------------------------------------------------
_PREFIX = 'module.'


def strip_prefix(state_dict):
    return {(k[len(_PREFIX):] if k.startswith(_PREFIX) else k): v for k, v in state_dict.items()}


def add_prefix(state_dict):
    return {_PREFIX + k: v for k, v in state_dict.items()}


# ---- exchange of the flat Adam moments with torch.optim.Adam (the reference's checkpoint format) -----------------------
def adam_state_to_torch(params, m, v, step, lr, betas, eps):
    """torch.optim.Adam's state_dict over `params` (flat-buffer order) from the flat moment buffers m, v."""
    state, off = {}, 0
    for i, p in enumerate(params):
        k = p.numel()
        state[i] = {'step': torch.tensor(float(step)), 'exp_avg': m[off:off + k].view(p.shape).clone(),
                    'exp_avg_sq': v[off:off + k].view(p.shape).clone()}
        off += k
    assert off == m.numel()
    group = {'lr': lr, 'betas': tuple(betas), 'eps': eps, 'weight_decay': 0, 'amsgrad': False,
             'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
             'decoupled_weight_decay': False, 'params': list(range(len(state)))}
    return {'state': state if step > 0 else {}, 'param_groups': [group]}


def adam_state_from_torch(params, m, v, opt_or_state_dict):
    """Fill m, v from a torch.optim.Adam (or its state_dict) over the same parameters -> (step count, lr); lr is None for a
    state_dict without `param_groups` (a caller that keeps its own rate, CascadeTrainer, accepts such a one)."""
    sd = opt_or_state_dict.state_dict() if hasattr(opt_or_state_dict, 'state_dict') else opt_or_state_dict
    st = sd['state']
    lr = float(sd['param_groups'][0]['lr']) if 'param_groups' in sd else None
    if len(st) == 0:
        m.zero_(); v.zero_()
        return 0, lr
    # a parameter that never received a gradient has NO entry in torch.optim.Adam's state (e.g. the unused views_linears.0 of
    # a reference checkpoint trained without view directions, model.py:60-61): zero moments, step count from the others
    off, steps = 0, set()
    for i, p in enumerate(params):
        k = p.numel()
        e = st.get(i)
        if e is None:
            m[off:off + k].zero_(); v[off:off + k].zero_()
        else:
            m[off:off + k].copy_(torch.as_tensor(e['exp_avg']).reshape(-1))
            v[off:off + k].copy_(torch.as_tensor(e['exp_avg_sq']).reshape(-1))
            steps.add(int(float(e['step'])))
        off += k
    assert off == m.numel() and len(steps) == 1, 'optimizer state does not match the parameter list'
    return steps.pop(), lr
