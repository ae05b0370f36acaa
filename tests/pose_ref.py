"""References for the pose-table kernels of csrc/pose.hip (pose_exp, pose_exp_bwd, pose_grad).

float64: torch.matrix_exp and its autograd (exp_ref64 / exp_bwd_ref64), the closed forms of include/fastnerf.h in float64
(closed_exp / closed_bwd), and the per-image sums of pose_grad with the bound of absolute values beside them (pose_grad_ref64).
float32: a numpy restatement of the kernels' formulas, operation by operation, every product and sum rounded on its own
(exp_f32 / exp_bwd_f32) -- what the arithmetic can give when sin, sqrt and the division are correctly rounded.

Inputs are always the fp32 values the kernels get; the references widen them."""
import numpy as np
import torch

THETAS = [0.0, 1e-30, 1e-12, 1e-8, 1e-4, 9e-4, 1.1e-3, 1e-2, 0.1, 0.49, 0.51, 1.0, 2.0, 3.0, float(np.pi)]
BOUND = 32.0 * 2.0 ** -24      # the cap of the issue: 32 ulp of 1, not a measurement
SERIES_AB, SERIES_C = 1e-3, 0.5


def hat(w):
    """[..., 3] -> [..., 3, 3], hat(w) x = w cross x."""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def random_rotations(n, gen):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    q[:, :, 0] *= torch.linalg.det(q)[:, None]
    return q


def exp_inputs(n_img, seed=0, first=0):
    """(base [n_img,3,4], xi [n_img,6], d_poses [n_img,3,4]) in fp32: random base rotations and axes, the rotation angles cycle through
    THETAS (image i has THETAS[(first + i) % 15]), normal translations and cotangents."""
    gen = torch.Generator().manual_seed(seed)
    base = torch.cat([random_rotations(n_img, gen), torch.randn(n_img, 3, 1, generator=gen, dtype=torch.float64) * 3], -1).float()
    axis = torch.randn(n_img, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    th = torch.tensor([THETAS[(first + i) % len(THETAS)] for i in range(n_img)], dtype=torch.float64)
    xi = torch.cat([axis * th[:, None], torch.randn(n_img, 3, generator=gen, dtype=torch.float64)], -1).float()
    return base, xi, torch.randn(n_img, 3, 4, generator=gen)


def exp_cases(n_img, seed=0):
    """The calls that put every theta of THETAS into a table of n_img images: [(base, xi, d_poses)]."""
    return [exp_inputs(n_img, seed + first, first) for first in range(0, len(THETAS), min(n_img, len(THETAS)))]


def exp_ref64(base, xi):
    """poses [n,3,4] float64: (matrix_exp(hat(omega)) R0 | t0 + tau)."""
    base, xi = base.double(), xi.double()
    R = torch.matrix_exp(hat(xi[:, :3])) @ base[:, :, :3]
    return torch.cat([R, base[:, :, 3:] + xi[:, 3:, None]], -1)


def exp_bwd_ref64(base, xi, d_poses):
    """d_xi [n,6] float64 by autograd of exp_ref64."""
    x = xi.double().clone().requires_grad_(True)
    return torch.autograd.grad((exp_ref64(base, x) * d_poses.double()).sum(), x)[0]


def _coefficients64(th2):
    """a, b, c of theta^2 in float64, each where it neither cancels nor divides by zero (series below 1e-2 / 0.5)."""
    th = th2.sqrt()
    small = th < 1e-2
    ths = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, 1 - th2 / 6 + th2 * th2 / 120 - th2 ** 3 / 5040, torch.sin(ths) / ths)
    h = ths / 2
    sh = torch.where(small, 1 - th2 / 24 + th2 * th2 / 1920, torch.sin(h) / h)
    b = 0.5 * sh * sh
    x = th2
    series = 1 / 6 - x / 120 + x ** 2 / 5040 - x ** 3 / 362880 + x ** 4 / 39916800 - x ** 5 / 6227020800 + x ** 6 / 1307674368000
    thc = torch.where(th < 0.5, torch.ones_like(th), th)
    c = torch.where(th < 0.5, series, (thc - torch.sin(thc)) / thc ** 3)
    return a, b, c


def closed_exp(base, xi):
    """The closed form of include/fastnerf.h in float64: R = I + a K + b K^2."""
    base, xi = base.double(), xi.double()
    w = xi[:, :3]
    a, b, _ = _coefficients64((w * w).sum(-1))
    K = hat(w)
    R = torch.eye(3, dtype=torch.float64) + a[:, None, None] * K + b[:, None, None] * (K @ K)
    return torch.cat([R @ base[:, :, :3], base[:, :, 3:] + xi[:, 3:, None]], -1)


def closed_bwd(base, xi, d_poses):
    """d_omega = J_l^T sum_k (A_k x G_k), J_l = I + b K + c K^2; d_tau = column 3 -- in float64."""
    base, xi, g = base.double(), xi.double(), d_poses.double()
    w = xi[:, :3]
    _, b, c = _coefficients64((w * w).sum(-1))
    A = closed_exp(base, xi)[:, :, :3]
    s = torch.cross(A, g[:, :, :3], dim=1).sum(-1)      # columns: the cross product runs over the row index
    K = hat(w)
    J = torch.eye(3, dtype=torch.float64) + b[:, None, None] * K + c[:, None, None] * (K @ K)
    return torch.cat([(J.transpose(1, 2) @ s[..., None])[..., 0], g[:, :, 3]], -1)


# ---- the kernels' arithmetic in numpy float32 ------------------------------------------------------------------------------------
F = np.float32


def _sinc32(x, x2):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(x < F(SERIES_AB), (F(1) - x2 * F(1 / 6)) + (x2 * x2) * F(1 / 120), np.sin(x) / x).astype(F)


def _rodrigues32(th2):
    th = np.sqrt(th2)
    a = _sinc32(th, th2)
    sh = _sinc32(F(0.5) * th, F(0.25) * th2)
    b = F(0.5) * (sh * sh)
    s = F(1 / 5040) - th2 * F(1 / 362880)
    s = F(1 / 120) - th2 * s
    series = F(1 / 6) - th2 * s
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.where(th < F(SERIES_C), series, (th - np.sin(th)) / (th2 * th)).astype(F)
    return a, b, c


def _compose32(base, w, th2, a, b):
    n = base.shape[0]
    R = np.zeros((n, 3, 3), F)
    for j in range(3):
        for k in range(3):
            ww = w[:, j] * w[:, k]
            R[:, j, k] = (F(1) + b * (ww - th2)) if j == k else b * ww
    aw = a[:, None] * w
    R[:, 0, 1] -= aw[:, 2]; R[:, 0, 2] += aw[:, 1]
    R[:, 1, 0] += aw[:, 2]; R[:, 1, 2] -= aw[:, 0]
    R[:, 2, 0] -= aw[:, 1]; R[:, 2, 1] += aw[:, 0]
    A = np.zeros((n, 3, 3), F)
    for j in range(3):
        for k in range(3):
            A[:, j, k] = (R[:, j, 0] * base[:, 0, k] + R[:, j, 1] * base[:, 1, k]) + R[:, j, 2] * base[:, 2, k]
    zero = th2 == 0
    A[zero] = base[zero][:, :, :3]
    return A


def exp_f32(base, xi):
    base, xi = base.numpy().astype(F), xi.numpy().astype(F)
    w = xi[:, :3]
    th2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    a, b, _ = _rodrigues32(th2)
    return torch.from_numpy(np.concatenate([_compose32(base, w, th2, a, b), (base[:, :, 3] + xi[:, 3:])[..., None]], -1))


def exp_bwd_f32(base, xi, d_poses):
    base, xi, g = base.numpy().astype(F), xi.numpy().astype(F), d_poses.numpy().astype(F)
    w = xi[:, :3]
    th2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    a, b, c = _rodrigues32(th2)
    A = _compose32(base, w, th2, a, b)
    s = np.zeros((base.shape[0], 3), F)
    for k in range(3):
        ax, ay, az, gx, gy, gz = A[:, 0, k], A[:, 1, k], A[:, 2, k], g[:, 0, k], g[:, 1, k], g[:, 2, k]
        s[:, 0] += ay * gz - az * gy
        s[:, 1] += az * gx - ax * gz
        s[:, 2] += ax * gy - ay * gx
    ws = (w[:, 0] * s[:, 0] + w[:, 1] * s[:, 1]) + w[:, 2] * s[:, 2]
    wxs = np.stack([w[:, 1] * s[:, 2] - w[:, 2] * s[:, 1], w[:, 2] * s[:, 0] - w[:, 0] * s[:, 2], w[:, 0] * s[:, 1] - w[:, 1] * s[:, 0]], -1)
    out = np.zeros((base.shape[0], 6), F)
    for j in range(3):
        kk = w[:, j] * ws - th2 * s[:, j]
        out[:, j] = (s[:, j] - b * wxs[:, j]) + c * kk
        out[:, 3 + j] = g[:, j, 3]
    return torch.from_numpy(out)


# ---- pose_grad -------------------------------------------------------------------------------------------------------------------
def dirs_of(pix, K, dtype=torch.float64):
    fx, fy, cx, cy = (np.float32(K[0][0]), np.float32(K[1][1]), np.float32(K[0][2]), np.float32(K[1][2]))
    row, col = pix[:, 1].numpy().astype(F), pix[:, 2].numpy().astype(F)
    d = np.stack([(col - cx) / fx, -(row - cy) / fy, -np.ones_like(col)], -1)      # the kernels' fp32 directions
    return torch.from_numpy(d).to(dtype)


def pose_grad_ref64(pix, poses, K, d_rays):
    """(d_poses [n_img,3,4], B [n_img,3,4], counts [n_img]) in float64: the sums of include/fastnerf.h, and the same sums with
    every factor replaced by its absolute value."""
    n_img = poses.shape[0]
    img = pix[:, 0].long()
    dirs = dirs_of(pix, K)
    R = poses.double()[img][:, :, :3]
    d = (R @ dirs[..., None])[..., 0]
    nrm = d.norm(dim=-1, keepdim=True)
    v = d / nrm
    g = d_rays.double()
    d_o, d_d, d_v = g[:, 0:3], g[:, 3:6], g[:, 8:11]
    g_d = d_d + (d_v - v * (v * d_v).sum(-1, keepdim=True)) / nrm
    a_d = d_d.abs() + (d_v.abs() + v.abs() * (v.abs() * d_v.abs()).sum(-1, keepdim=True)) / nrm
    rows = torch.cat([g_d[:, :, None] * dirs[:, None, :], d_o[:, :, None]], -1)
    rows_abs = torch.cat([a_d[:, :, None] * dirs.abs()[:, None, :], d_o.abs()[:, :, None]], -1)
    out = torch.zeros(n_img, 3, 4, dtype=torch.float64).index_add_(0, img, rows)
    B = torch.zeros(n_img, 3, 4, dtype=torch.float64).index_add_(0, img, rows_abs)
    return out, B, torch.bincount(img, minlength=n_img)


def exact_case(n, n_img, empty=(), seed=0):
    """The integer case of the issue: fx = fy = 1, cx = cy = 0, rows / cols < 8, permutation poses, d_v = 0, integer d_o and d_d in
    [-2, 2]: every term is an integer of magnitude <= 14 and every partial sum stays below 2^24 (n <= 2^24 / 14), so any order of fp32
    sums gives the int64 sum.  -> (pix int32 [n,3], poses [n_img,3,4], K, d_rays [n,11], want int64 [n_img,3,4])"""
    gen = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([i for i in range(n_img) if i not in empty])
    pix = torch.stack([allowed[torch.randint(0, len(allowed), (n,), generator=gen)], torch.randint(0, 8, (n,), generator=gen),
                       torch.randint(0, 8, (n,), generator=gen)], 1).int()
    perms = torch.tensor([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])
    poses = torch.zeros(n_img, 3, 4)
    for i in range(n_img):
        poses[i, torch.arange(3), perms[i % 6]] = 1.0 if i % 2 == 0 else -1.0
        poses[i, :, 3] = float(i)
    K = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    d_rays = torch.zeros(n, 11)
    d_rays[:, 0:6] = torch.randint(-2, 3, (n, 6), generator=gen).float()
    d_rays[:, 6:8] = torch.randn(n, 2, generator=gen)      # ignored by the kernel
    dirs = torch.stack([pix[:, 2], -pix[:, 1], -torch.ones_like(pix[:, 1])], -1).long()
    rows = torch.cat([d_rays[:, 3:6].long()[:, :, None] * dirs[:, None, :], d_rays[:, 0:3].long()[:, :, None]], -1)
    want = torch.zeros(n_img, 3, 4, dtype=torch.int64).index_add_(0, pix[:, 0].long(), rows)
    return pix, poses, K, d_rays, want


def float_case(n, n_img, empty=(), seed=0):
    """800 x 800 cameras, random poses (rotation, normal translation), Gaussian d_rays."""
    gen = torch.Generator().manual_seed(seed)
    allowed = torch.tensor([i for i in range(n_img) if i not in empty])
    pix = torch.stack([allowed[torch.randint(0, len(allowed), (n,), generator=gen)], torch.randint(0, 800, (n,), generator=gen),
                       torch.randint(0, 800, (n,), generator=gen)], 1).int()
    poses = torch.cat([random_rotations(n_img, gen), torch.randn(n_img, 3, 1, generator=gen, dtype=torch.float64)], -1).float()
    K = [[1111.0, 0.0, 400.0], [0.0, 1111.0, 400.0], [0.0, 0.0, 1.0]]
    return pix, poses, K, torch.randn(n, 11, generator=gen)
