"""CPU: the fp64 restatement of matrix_to_quaternion that the GPU pose-codec test uses as its reference (tests/pose_codec_checks.py)
is the inverse of the oracle's quaternion_to_matrix on every case, returns unit quaternions with a non-negative real part, and takes
every one of its four candidate branches."""
import torch

from oracle import pd_oracle as O
from pose_codec_checks import camera_to_pose_encoding, matrix_to_quaternion, rotation_cases


def test_matrix_to_quaternion_restatement_inverts_the_oracle():
    cases = rotation_cases()
    assert len(cases) == 64 + 1 + 4 + 2
    taken = {}
    for name, q in cases:
        R = O.quaternion_to_matrix(q)
        mq, branch = matrix_to_quaternion(R, return_branch=True)
        taken[name] = int(branch)
        assert (O.quaternion_to_matrix(mq) - R).abs().max() < 1e-12, name
        assert abs(float(mq.norm()) - 1.0) < 1e-12, name
        assert float(mq[0]) >= 0.0, name
        assert min((mq - q).abs().max(), (mq + q).abs().max()) < 1e-12, name
    # real part 0: a non-real candidate each -- x, y, z; the tie of (1, 1, 0) / sqrt 2 goes to one of its two equal candidates
    assert taken["pi_x"] == 1 and taken["pi_y"] == 2 and taken["pi_z"] == 3 and taken["pi_xy"] in (1, 2), taken
    assert taken["identity"] == 0 and taken["tiny"] == 0 and taken["almost_pi"] != 0, taken
    assert {taken[f"random{i}"] for i in range(64)} == {0, 1, 2, 3}, taken


def test_matrix_to_quaternion_restatement_is_batched():
    q = torch.stack([c[1] for c in rotation_cases()])
    R = O.quaternion_to_matrix(q)
    one = torch.stack([matrix_to_quaternion(R[i]) for i in range(len(R))])
    assert torch.equal(matrix_to_quaternion(R), one)
    assert torch.equal(matrix_to_quaternion(R[:70].reshape(7, 10, 3, 3)).reshape(-1, 4), one[:70])


def test_camera_to_pose_encoding_restatement_layout_and_clamp():
    R = O.quaternion_to_matrix(torch.stack([c[1] for c in rotation_cases()[:3]]))
    T = torch.arange(9, dtype=torch.float64).reshape(3, 3)
    focal = torch.tensor([[0.01, 1.0], [3.0, 300.0], [2.0, 2.0]], dtype=torch.float64)
    enc = camera_to_pose_encoding(R, T, focal, 1.5, 0.2, 10.0)
    assert enc.shape == (3, 9) and torch.equal(enc[:, :3], T) and torch.equal(enc[:, 3:7], matrix_to_quaternion(R))
    want = torch.log(torch.tensor([[0.2, 1.0], [3.0, 10.0], [2.0, 2.0]], dtype=torch.float64)) - 1.5
    assert (enc[:, 7:] - want).abs().max() < 1e-15
