"""camera_to_pose_encoding (util/camera_transform.py:108-129) in float64, and the cases its tests run.

pytorch3d is not a dependency of this project and the oracle stubs the reference's import of `matrix_to_quaternion` to None, so no
reference-generated fixture exists for this one function: the yardstick is the restatement below of current pytorch3d's rule
(transforms/rotation_conversions.py), validated on the CPU against the oracle's quaternion_to_matrix by
tests/test_pose_codec_checks_cpu.py and used as the fp64 reference by tests/test_gpu_pose_codec.py.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch


def matrix_to_quaternion(R: torch.Tensor, return_branch: bool = False):
    """[.., 3, 3] -> [.., 4] (real part first): the four candidates q_abs = sqrt(max(0, 1 +- m00 +- m11 +- m22)), the candidate row of
    the largest q_abs divided by 2 max(q_abs, 0.1), standardised to a non-negative real part.  ``return_branch``: also the index of
    the candidate taken (0 = the real part is the largest component, 1..3 = i, j, k)."""
    R = torch.as_tensor(R)
    m = R.reshape(R.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(m, -1)
    s = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], dim=-1)
    q_abs = torch.where(s > 0, torch.sqrt(s.clamp_min(0)), torch.zeros_like(s))
    cand = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1),
    ], dim=-2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    branch = q_abs.argmax(dim=-1)
    q = torch.gather(cand, -2, branch[..., None, None].expand(branch.shape + (1, 4))).squeeze(-2)
    q = torch.where(q[..., :1] < 0, -q, q)
    return (q, branch) if return_branch else q


def camera_to_pose_encoding(R, T, focal, log_focal_length_bias=1.8, min_focal_length=0.1, max_focal_length=20.0) -> torch.Tensor:
    """[n, 9] = [T | matrix_to_quaternion(R) | log(clamp(focal)) - bias] in the dtype of the inputs (camera_transform.py:113-124)."""
    R, T, focal = torch.as_tensor(R), torch.as_tensor(T), torch.as_tensor(focal)
    logfl = torch.log(torch.clamp(focal, min=min_focal_length, max=max_focal_length)) - log_focal_length_bias
    return torch.cat([T.reshape(-1, 3), matrix_to_quaternion(R.reshape(-1, 3, 3)), logfl.reshape(-1, 2)], dim=-1)


def _axis_angle_quat(axis, angle: float) -> torch.Tensor:
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    return torch.cat([torch.tensor([math.cos(0.5 * angle)], dtype=torch.float64), math.sin(0.5 * angle) * a])


def rotation_cases() -> List[Tuple[str, torch.Tensor]]:
    """(name, unit quaternion [4] float64) of every case: 64 random rotations, the identity, 180 degrees about x, y, z and about
    (1, 1, 0) / sqrt 2 (real part 0: the three non-real candidates), 179.99 degrees, and 1e-4 rad."""
    g = torch.Generator().manual_seed(2024)
    q = torch.randn(64, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=-1, keepdim=True)
    cases = [(f"random{i}", q[i]) for i in range(64)]
    cases.append(("identity", torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)))
    for name, axis in (("pi_x", (1, 0, 0)), ("pi_y", (0, 1, 0)), ("pi_z", (0, 0, 1)), ("pi_xy", (1, 1, 0))):
        cases.append((name, _axis_angle_quat(axis, math.pi)))
    cases.append(("almost_pi", _axis_angle_quat((0.3, -0.5, 0.8), math.radians(179.99))))
    cases.append(("tiny", _axis_angle_quat((-0.6, 0.2, 0.7), 1e-4)))
    return cases


def camera_cases(n_repeat: int = 1) -> Dict[str, torch.Tensor]:
    """Cameras of every rotation case (float64): R [n, 3, 3] from the oracle's quaternion_to_matrix, T ~ N(0, 3), focal lengths inside
    [0.1, 20] for all but the last four cameras of a repeat, which sit outside the range on either side (0.01, 0.05 / 25, 300)."""
    from oracle import pd_oracle as O
    q = torch.stack([c[1] for c in rotation_cases()]).repeat(n_repeat, 1)
    n = q.shape[0]
    g = torch.Generator().manual_seed(77)
    T = 3.0 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    focal = torch.exp(torch.empty(n, 2, dtype=torch.float64).uniform_(math.log(0.12), math.log(19.0), generator=g))
    inside = torch.ones(n, dtype=torch.bool)
    per = n // n_repeat
    for r in range(n_repeat):
        focal[r * per + per - 4] = torch.tensor([0.01, 1.0], dtype=torch.float64)
        focal[r * per + per - 3] = torch.tensor([2.0, 0.05], dtype=torch.float64)
        focal[r * per + per - 2] = torch.tensor([25.0, 3.0], dtype=torch.float64)
        focal[r * per + per - 1] = torch.tensor([300.0, 0.02], dtype=torch.float64)
        inside[r * per + per - 4:r * per + per] = False
    return {"q": q, "R": O.quaternion_to_matrix(q), "T": T, "focal": focal, "inside": inside}
