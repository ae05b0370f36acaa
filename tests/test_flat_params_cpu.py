"""flat_params.py on the host: the flat-buffer layout of the four network shapes, their seeded initialisation, the slice functions'
return types, the Adam-state exchange with torch.optim.Adam and the checkpoint prefix.  No GPU: the constructors only allocate
on the device they are given, and ops.net_floats is a host call into the library."""
import pytest
import torch
from torch import nn

import fastnerf
from fastnerf import flat_params, ops
from fastnerf.model import NeRF, noview_slices, param_slices
from fastnerf.nerfpp import MLPNet, mlpnet_slices


def _trunk(ic):
    return [(ic, 256)] + [(256, 256)] * 4 + [(256 + ic, 256)] + [(256, 256)] * 2


# name -> (constructor, slice table, nn.Linear (in, out) in the order the class documents: the reference's construction order)
NETS = {
    'nerf': (lambda: NeRF(use_viewdirs=True, device='cpu'), param_slices,
             _trunk(63) + [(283, 128), (256, 256), (256, 1), (128, 3)]),
    'nerf_noview': (lambda: NeRF(use_viewdirs=False, input_ch_views=0, output_ch=5, device='cpu'), lambda: noview_slices(5)[0],
                    _trunk(63) + [(256, 128), (256, 5)]),
    'mlpnet_fg': (lambda: MLPNet(input_ch=63, device='cpu'), lambda: mlpnet_slices(1),
                  _trunk(63) + [(256, 1), (256, 256), (283, 128), (128, 3)]),
    'mlpnet_bg': (lambda: MLPNet(input_ch=84, device='cpu'), lambda: mlpnet_slices(2),
                  _trunk(84) + [(256, 1), (256, 256), (283, 128), (128, 3)]),
}


def _buffers(net):
    """(parameters, gradients) in parameters() order: what the parameters are views of."""
    return getattr(net, 'param_flat', net.flat), getattr(net, 'param_grad', net.flat_grad)


@pytest.fixture(scope='module')
def nets():
    out = {}
    for name, (make, _, _) in NETS.items():
        torch.manual_seed(0)
        out[name] = make()
    return out


@pytest.mark.parametrize('name', list(NETS))
def test_layout(nets, name):
    net, table = nets[name], NETS[name][1]()
    flat, grad = _buffers(net)
    params = list(net.named_parameters())
    assert [n for n, _ in params] == [n for n, _, _ in table]
    end = 0
    for (_, p), (_, off, shape) in zip(params, table):
        assert off == end, 'slices are contiguous'
        assert tuple(p.shape) == tuple(shape)
        assert p.data_ptr() == flat.data_ptr() + 4 * off
        assert p.grad.data_ptr() == grad.data_ptr() + 4 * off and p.grad.shape == p.shape
        end = off + p.numel()
    assert end == flat.numel() == grad.numel()
    assert end == {'nerf': 595844, 'nerf_noview': 527237, 'mlpnet_fg': 595844, 'mlpnet_bg': ops.net_floats(2, 0)}[name]
    assert end == sum(i * o + o for i, o in NETS[name][2])
    assert net.flat.numel() == ops.net_floats(getattr(net, 'kind', 0), 0)       # what the kernels read


@pytest.mark.parametrize('name', list(NETS))
def test_seeded_init(nets, name):
    torch.manual_seed(0)
    layers = [nn.Linear(i, o) for i, o in NETS[name][2]]
    want = torch.cat([t.detach().reshape(-1) for l in layers for t in (l.weight, l.bias)])
    assert torch.equal(_buffers(nets[name])[0], want)


def test_slice_function_types():
    s = param_slices()
    assert isinstance(s, list) and len(s) == 24 and s[0] == ('pts_linears.0.weight', 0, (256, 63))
    pair = noview_slices(4)
    assert isinstance(pair, tuple) and len(pair) == 2
    assert isinstance(pair[0], list) and len(pair[0]) == 20 and isinstance(pair[1], int)
    assert pair[1] == pair[0][-1][1] + 4
    for kind in (1, 2):
        s = mlpnet_slices(kind)
        assert isinstance(s, list) and len(s) == 24 and s[0] == ('base_layers.0.0.weight', 0, (256, 63 if kind == 1 else 84))
    assert flat_params.slices([('a', (2, 3)), ('b', (1, 2))]) == (
        [('a.weight', 0, (2, 3)), ('a.bias', 6, (2,)), ('b.weight', 8, (1, 2)), ('b.bias', 10, (1,))], 11)
    v = flat_params.views(torch.arange(11.), flat_params.slices([('a', (2, 3)), ('b', (1, 2))])[0])
    assert list(v) == ['a.weight', 'a.bias', 'b.weight', 'b.bias'] and v['b.weight'].tolist() == [[8., 9.]]


# ---- Adam exchange -------------------------------------------------------------------------------------------------------
SHAPES = [(3, 4), (3,), (2, 3)]
N = 12 + 3 + 6


def _adam_case():
    g = torch.Generator().manual_seed(1)
    params = [nn.Parameter(torch.rand(s, generator=g)) for s in SHAPES]
    return params, torch.rand(N, generator=g), torch.rand(N, generator=g)


def _to_torch(params, m, v, step=7):
    return flat_params.adam_state_to_torch(params, m, v, step, 2e-4, (0.9, 0.999), 1e-8)


def test_adam_round_trip_through_torch_optimizer():
    params, m, v = _adam_case()
    sd = _to_torch(params, m, v)
    for i, p in enumerate(params):
        e = sd['state'][i]
        assert e['exp_avg'].shape == p.shape and e['exp_avg_sq'].shape == p.shape
        assert e['exp_avg'].data_ptr() != m.data_ptr() + 4 * sum(q.numel() for q in params[:i]), 'clones, not views'
        assert torch.equal(e['step'], torch.tensor(7.0))
    opt = torch.optim.Adam([nn.Parameter(torch.zeros(s)) for s in SHAPES], lr=1.0)
    opt.load_state_dict(sd)
    for src in (opt, opt.state_dict(), sd):
        m2, v2 = torch.full((N,), -1.0), torch.full((N,), -1.0)
        step, lr = flat_params.adam_state_from_torch(params, m2, v2, src)
        assert step == 7 and isinstance(step, int) and lr == 2e-4
        assert torch.equal(m2, m) and torch.equal(v2, v)


def test_adam_step_zero_is_an_empty_state():
    params, m, v = _adam_case()
    sd = _to_torch(params, m, v, step=0)
    assert sd['state'] == {} and sd['param_groups'][0]['params'] == [0, 1, 2]
    torch.optim.Adam([nn.Parameter(torch.zeros(s)) for s in SHAPES]).load_state_dict(sd)
    assert flat_params.adam_state_from_torch(params, m, v, sd) == (0, 2e-4)
    assert not m.any() and not v.any()


def test_adam_state_dict_without_param_groups():
    """CascadeTrainer.load_torch_optimizer never read `param_groups`: a dict with `state` alone loads, lr is None."""
    params, m, v = _adam_case()
    sd = {'state': _to_torch(params, m, v)['state']}
    m2, v2 = torch.zeros(N), torch.zeros(N)
    assert flat_params.adam_state_from_torch(params, m2, v2, sd) == (7, None)
    assert torch.equal(m2, m) and torch.equal(v2, v)


def test_adam_missing_entry_zeroes_that_parameter_only():
    params, m, v = _adam_case()
    sd = _to_torch(params, m, v)
    del sd['state'][1]
    m2, v2 = torch.full((N,), -1.0), torch.full((N,), -1.0)
    assert flat_params.adam_state_from_torch(params, m2, v2, sd) == (7, 2e-4)
    keep = torch.ones(N, dtype=torch.bool)
    keep[12:15] = False
    assert torch.equal(m2[keep], m[keep]) and torch.equal(v2[keep], v[keep])
    assert not m2[12:15].any() and not v2[12:15].any()


def test_adam_mismatches_raise():
    params, m, v = _adam_case()
    sd = _to_torch(params, m, v)
    sd['state'][2]['step'] = torch.tensor(8.0)
    with pytest.raises(AssertionError, match='optimizer state does not match the parameter list'):
        flat_params.adam_state_from_torch(params, m.clone(), v.clone(), sd)
    sd = _to_torch(params, m, v)
    with pytest.raises(AssertionError, match='optimizer state does not match the parameter list'):
        flat_params.adam_state_from_torch(params, torch.zeros(N + 1), torch.zeros(N + 1), sd)
    with pytest.raises(AssertionError):
        flat_params.adam_state_to_torch(params, torch.zeros(N + 1), torch.zeros(N + 1), 7, 2e-4, (0.9, 0.999), 1e-8)


def test_adam_param_group_is_the_reference_format():
    params, m, v = _adam_case()
    lr, beta1, beta2, eps, state = 2e-4, 0.9, 0.999, 1e-8, range(3)
    # the dict the two trainers wrote before this module existed, copied from their code
    group = {'lr': lr, 'betas': (beta1, beta2), 'eps': eps, 'weight_decay': 0, 'amsgrad': False,
             'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
             'decoupled_weight_decay': False, 'params': list(range(len(state)))}
    sd = _to_torch(params, m, v)
    assert list(sd) == ['state', 'param_groups'] and len(sd['param_groups']) == 1
    got = sd['param_groups'][0]
    assert list(got) == list(group)
    for k in group:
        assert got[k] == group[k] and type(got[k]) is type(group[k]), k


# ---- checkpoint prefix ---------------------------------------------------------------------------------------------------
def test_prefix_helpers(nets):
    sd = {'pts_linears.0.weight': 1, 'module_x': 2, 'a.module.b': 3}
    pre = flat_params.add_prefix(sd)
    assert list(pre) == ['module.pts_linears.0.weight', 'module.module_x', 'module.a.module.b']
    assert flat_params.strip_prefix(pre) == sd and list(flat_params.strip_prefix(pre)) == list(sd)
    assert flat_params.strip_prefix(sd) == sd                  # keys without the prefix pass through
    net = nets['nerf']
    ref = fastnerf.run_nerf.reference_state_dict(net)
    assert list(ref) == ['module.' + k for k in net.state_dict()]
    assert all(ref['module.' + k] is v or ref['module.' + k].data_ptr() == v.data_ptr() for k, v in net.state_dict().items())
    before = _buffers(net)[0].clone()
    net.load_state_dict(ref)                                   # with the prefix
    net.load_state_dict(net.state_dict())                      # and without
    assert torch.equal(_buffers(net)[0], before)
