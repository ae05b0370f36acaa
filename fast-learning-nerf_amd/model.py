"""NeRF MLP (mirror of nerf-ours/model.py:8-63) whose parameters are views into ONE flat
fp32 buffer laid out in `model.parameters()` order, so that

  * the HIP kernels (fastnerf_mlp_fwd / _bwd / adam_step) work on the flat buffer directly,
  * `state_dict()` keeps the reference's names (pts_linears.{0..7}, views_linears.0,
    feature_linear, alpha_linear, rgb_linear) and `load_state_dict` of a reference
    checkpoint (with or without the DataParallel `module.` prefix) just works,
  * a data-parallel all-reduce is a single collective over `flat_grad`.

What that layout means -- slice table, views, binding, packed-weight cache, checkpoint prefix -- is written once in
flat_params.py; this module supplies the shapes.

The kernels implement the configuration the reference's configs use (D=8, W=256, skips=[4], use_viewdirs=True,
input_ch=63, input_ch_views=27).  `use_viewdirs=False` (model.py:35-36,60-61: one `output_linear` 256 -> output_ch on the
trunk, no view branch) runs on the SAME kernels through an exactly equivalent view-branch network (`NeRF._sync_kernel_net`):
feature layer = identity, view layer rows (2c, 2c+1) = (+w_c, -w_c) of output row c with zero weights on the direction
encoding, colour head = relu(a) - relu(-a) = a, sigma head = output row 3.  In fp32 arithmetic every one of those steps is
exact (products with 0 / 1, one non-zero term per sum), so the result is the reference's dot product; the parameters,
their names, order and gradients are the reference's (`views_linears.0` exists there too, unused).
"""
import torch
from torch import nn

from . import flat_params, ops

SHAPES = (
    [(f'pts_linears.{i}', (256, 63 if i == 0 else (319 if i == 5 else 256))) for i in range(8)]
    + [('views_linears.0', (128, 283)), ('feature_linear', (256, 256)), ('alpha_linear', (1, 256)),
       ('rgb_linear', (3, 128))]
)


def noview_shapes(output_ch):
    """Modules of the reference model without view directions in registration order (model.py:20-36, input_ch_views = 0)."""
    return SHAPES[:8] + [('views_linears.0', (128, 256)), ('output_linear', (output_ch, 256))]


def noview_slices(output_ch):
    """[(name, offset, shape)], total floats -- parameters() order of the model without view directions."""
    return flat_params.slices(noview_shapes(output_ch))


PTS_FLOATS = sum(o * i + o for _, (o, i) in SHAPES[:8])   # the trunk comes first in both layouts


def param_slices():
    """[(name, offset, shape)] in model.parameters() order."""
    out, off = flat_params.slices(SHAPES)
    assert off == ops.NET_PARAMS
    return out


class NeRF(flat_params.FlatNet):
    def __init__(self, D=8, W=256, input_ch=63, input_ch_views=27, output_ch=4, skips=[4], use_viewdirs=True,
                 device='cuda', flat=None, flat_grad=None):
        super().__init__()
        if not (D == 8 and W == 256 and input_ch == 63 and list(skips) == [4]
                and ((use_viewdirs and input_ch_views == 27) or (not use_viewdirs and input_ch_views == 0))):
            raise NotImplementedError('the HIP MLP implements D=8, W=256, input_ch=63, skips=[4] with input_ch_views=27 '
                                      '(use_viewdirs) or 0 (no view directions)')
        self.D, self.W, self.input_ch, self.input_ch_views = D, W, input_ch, input_ch_views
        self.skips, self.use_viewdirs, self.output_ch = list(skips), use_viewdirs, output_ch
        # same construction order as the reference => identical init under torch.manual_seed
        pts = nn.ModuleList([nn.Linear(input_ch, W)] +
                            [nn.Linear(W, W) if i not in self.skips else nn.Linear(W + input_ch, W)
                             for i in range(D - 1)])
        views = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        self.pts_linears, self.views_linears = pts, views
        if use_viewdirs:
            feature, alpha, rgb = nn.Linear(W, W), nn.Linear(W, 1), nn.Linear(W // 2, 3)
            self.feature_linear, self.alpha_linear, self.rgb_linear = feature, alpha, rgb
            slices, total = param_slices(), ops.NET_PARAMS
        else:
            if output_ch < 4:
                raise ValueError('output_ch must be >= 4 (rgb + sigma)')
            self.output_linear = nn.Linear(W, output_ch)
            slices, total = noview_slices(output_ch)
        dev = torch.device(device)
        pflat = flat if flat is not None else torch.empty(total, device=dev, dtype=torch.float32)
        pgrad = flat_grad if flat_grad is not None else torch.zeros(total, device=dev, dtype=torch.float32)
        assert pflat.numel() == total and pgrad.numel() == total
        flat_params.bind(self, slices, pflat, pgrad)
        self.param_flat, self.param_grad = pflat, pgrad      # the reference's parameters, parameters() order
        if use_viewdirs:
            self.flat, self.flat_grad = pflat, pgrad          # ... which is also what the kernels read / write
        else:
            # what the kernels read / write: the equivalent view-branch network (module docstring), standard layout
            self.flat = torch.zeros(ops.NET_PARAMS, device=dev, dtype=torch.float32)
            self.flat_grad = torch.zeros(ops.NET_PARAMS, device=dev, dtype=torch.float32)
            k = self._kernel_views(self.flat)
            k['feature_linear.weight'].copy_(torch.eye(256, device=dev))
            for c in range(3):
                k['rgb_linear.weight'][c, 2 * c] = 1.0
                k['rgb_linear.weight'][c, 2 * c + 1] = -1.0
            self._sync_kernel_net()

    # ---- no view directions: parameters <-> the equivalent view-branch network the kernels run -----------------
    @staticmethod
    def _kernel_views(flat):
        return flat_params.views(flat, param_slices())

    # ---- band weights: the kernels run the network whose encoding columns are the parameters' times w (bands.py) -------------
    _bands = None          # (w_pos [63], w_view [27]) on the device while band weights are set
    _band_host = None      # ... and on the host: an unchanged pair is not uploaded again
    _band_pool = None      # create_nerf: the dict its two networks share, so that their effective buffers are one allocation
    _band_slot = None      # ... and this network's slice of it

    def set_bands(self, w_pos, w_view, sync=True):
        """-> whether the weights differ from those that were set (they are uploaded only then).  sync=False leaves making `flat`
        current to the caller's next packed(refresh=True).  Weigh the columns of the point and direction encodings by w_pos [63] / w_view [27] (finite, in [0, 1]; bands.BandSchedule
        makes them): from now on `flat` / `flat_grad` are buffers of their own that hold the EFFECTIVE network -- the parameters with
        the encoding columns of layer 0, the skip layer and the view layer times w (ops.band_apply, run before every re-pack) -- and
        its gradient, while `param_flat` / `param_grad` stay what parameters() and their .grad view; `param_grads_from` and
        `collect_grads` carry a kernel gradient to the parameters (ops.band_grad).  Everything that reads `flat` and `packed()` sees
        the weighted field.  A column at weight 0 is neither read (its effective weights are 0) nor moved (its gradient is 0).
        ValueError for a network without view directions (its `flat` is derived already) and for weights that are none."""
        if not self.use_viewdirs:
            raise ValueError('NeRF.set_bands: a network without view directions already runs on a derived kernel network; band weights '
                             'need use_viewdirs=True')
        from .bands import check_weights
        host = check_weights(w_pos, w_view)
        if self._bands is None:
            dev = self.param_flat.device
            pool = self._band_pool
            if pool is None:
                self.flat, self.flat_grad = torch.empty_like(self.param_flat), torch.zeros_like(self.param_grad)
            else:
                if pool.get('flat') is None:
                    pool['flat'], pool['grad'] = torch.empty_like(pool['params']), torch.zeros_like(pool['params'])
                self.flat, self.flat_grad = pool['flat'][self._band_slot], pool['grad'][self._band_slot]
            self._bands = tuple(torch.empty_like(w, device=dev) for w in host)
            self._band_host = None
        changed = self._band_host is None or not all(torch.equal(a, b) for a, b in zip(host, self._band_host))
        if changed:
            for d, h in zip(self._bands, host):
                d.copy_(h)
            self._band_host = host
        if sync:
            self._sync_kernel_net()
        return changed

    def clear_bands(self):
        """Back to the network without band weights: `flat` / `flat_grad` are the parameters' buffers again (re-pack before the next
        use of a cached packed(refresh=False))."""
        if self._bands is not None:
            self._bands = self._band_host = None
            self.flat, self.flat_grad = self.param_flat, self.param_grad

    def _sync_kernel_net(self):
        if self._bands is not None:
            ops.band_apply(self._bands[0], self._bands[1], self.param_flat, self.flat)
        if self.use_viewdirs:
            return
        with torch.no_grad():
            k = self._kernel_views(self.flat)
            self.flat[:PTS_FLOATS].copy_(self.param_flat[:PTS_FLOATS])
            w, b = self.output_linear.weight, self.output_linear.bias
            vw, vb = k['views_linears.0.weight'], k['views_linears.0.bias']
            vw[0:6:2, :256] = w[:3]
            vw[1:6:2, :256] = -w[:3]
            vb[0:6:2] = b[:3]
            vb[1:6:2] = -b[:3]
            k['alpha_linear.weight'].copy_(w[3:4])
            k['alpha_linear.bias'].copy_(b[3:4])

    def param_grads_from(self, kernel_grad):
        """Gradients in parameters() order from a gradient buffer the kernels wrote (standard layout)."""
        if self._bands is not None:      # the effective network's gradient -> the parameters': the encoding columns times w, on a copy
            kernel_grad = ops.band_grad(self._bands[0], self._bands[1], kernel_grad.clone())
        k = self._kernel_views(kernel_grad)
        if self.use_viewdirs:
            return [k[name] for name, _, _ in param_slices()]
        out = []
        for name, _, shape in noview_slices(self.output_ch)[0]:
            if name.startswith('pts_linears.'):
                out.append(k[name])
            elif name.startswith('views_linears.'):          # never used by the forward pass (model.py:60-61)
                out.append(torch.zeros(shape, device=kernel_grad.device))
            else:
                vg = k['views_linears.0.weight'] if name.endswith('weight') else k['views_linears.0.bias']
                ag = k['alpha_linear.weight'] if name.endswith('weight') else k['alpha_linear.bias']
                g = torch.zeros(shape, device=kernel_grad.device)
                if name.endswith('weight'):
                    g[:3] = vg[0:6:2, :256] - vg[1:6:2, :256]
                else:
                    g[:3] = vg[0:6:2] - vg[1:6:2]
                g[3:4] = ag                                   # rows >= 4 (output_ch = 5) are never read: zero gradient
                out.append(g)
        return out

    def collect_grads(self):
        """After a backward that wrote `flat_grad`: make the parameters' .grad (views of `param_grad`) current."""
        if self._bands is not None:
            self.param_grad.copy_(self.flat_grad)
            ops.band_grad(self._bands[0], self._bands[1], self.param_grad)
        if self.use_viewdirs:
            return
        with torch.no_grad():
            for (name, off, shape), g in zip(noview_slices(self.output_ch)[0], self.param_grads_from(self.flat_grad)):
                self.param_grad[off:off + g.numel()].view(shape).copy_(g)

    def forward(self, x):
        """Reference signature: x = [.., 63 + 27] already-embedded inputs (model.py:38-63).
        Convenience path for third-party callers (e.g. mesh extraction); the renderer never
        calls it -- it runs the fused HIP kernels on raw rays instead."""
        F = torch.nn.functional
        pts, views = torch.split(x, [self.input_ch, self.input_ch_views], dim=-1)
        h = pts
        for i in range(self.D):
            h = F.relu(self.pts_linears[i](h))
            if i in self.skips:
                h = torch.cat([pts, h], -1)
        if not self.use_viewdirs:
            return self.output_linear(h)
        alpha = self.alpha_linear(h)
        h = torch.cat([self.feature_linear(h), views], -1)
        h = F.relu(self.views_linears[0](h))
        return torch.cat([self.rgb_linear(h), alpha], -1)

    def density_gradient(self, points, chunk=65536):
        """(sigma [...], grad [..., 3]) at `points` [..., 3] (a cuda tensor): the density logit raw[..., 3] of the fused forward
        under the current math mode and its gradient with respect to the point, both before the ReLU that turns the logit into a
        density (ops.mlp_sigma_grad).  -grad / |grad| is the surface normal of the field (mesh.vertex_normals).

        Runs under torch.no_grad(), `chunk` points at a time: the saved activations and pre-activation gradients of a chunk take
        about 20 KB per point, 1.3 GB at the default.  A network without view directions runs on its equivalent kernel network
        `self.flat`, whose sigma head is output row 3 (module docstring)."""
        if not torch.is_tensor(points):
            raise RuntimeError('fastnerf ops run on the GPU only (no CPU fallback): got a host array')
        ops.require_gpu(points)
        if points.shape[-1] != 3:
            raise ValueError('density_gradient needs points [..., 3], got shape %s' % (tuple(points.shape),))
        lead = tuple(points.shape[:-1])
        pts = points.detach().reshape(-1, 3).float()
        P = pts.shape[0]
        dev = pts.device
        sigma = torch.empty(P, device=dev, dtype=torch.float32)
        grad = torch.empty(P, 3, device=dev, dtype=torch.float32)
        if P == 0:
            return sigma.reshape(lead), grad.reshape(lead + (3,))
        n0 = min(max(1, int(chunk)), P)
        with torch.no_grad():
            pf, pb = self.packed()
            ws = torch.empty(ops.sigma_grad_ws_floats(n0), device=dev, dtype=torch.float32)
            rays11 = torch.zeros(n0, 11, device=dev, dtype=torch.float32)     # o = the point, d = 0: o + d * z is the point itself
            z = torch.zeros(n0, 1, device=dev, dtype=torch.float32)
            for p0 in range(0, P, n0):
                n = min(n0, P - p0)
                rays11[:n, 0:3] = pts[p0:p0 + n]
                s, _ = ops.mlp_sigma_grad(rays11[:n], z[:n], self.flat, pf, pb, ws=ws, grad=grad[p0:p0 + n])
                sigma[p0:p0 + n] = s[:, 0]
        return sigma.reshape(lead), grad.reshape(lead + (3,))

    def load_state_dict(self, state_dict, strict=True):
        return super().load_state_dict(flat_params.strip_prefix(state_dict), strict=strict)
