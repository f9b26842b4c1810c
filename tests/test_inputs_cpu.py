"""CPU tests of emap_amd/_inputs.py: what the post-training wrappers do to their arguments before a C call - device placement, the host copy
of a small matrix, the world-to-camera convention, the shape of the edge maps, the parametric_edges.json path-or-dict."""
import json
import pathlib

import numpy as np
import pytest
import torch

from emap_amd import _inputs

PTS = [[0.0, 1.0, 2.0], [3.0, 4.0, 5.5]]
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("make", [np.array, list, torch.tensor], ids=["numpy", "list", "tensor"])
def test_numpy_lists_and_tensors_become_contiguous_tensors_of_the_wanted_dtype(make):
    t = _inputs.to_device(make(PTS), "cpu")
    assert t.dtype == F64 and t.is_contiguous() and t.tolist() == PTS and t.device.type == "cpu"
    assert _inputs.to_device(make(PTS), "cpu", F32).dtype == F32
    assert _inputs.points(make(PTS), "cpu", "tag").dtype == F32                 # the fp32-keeping form makes everything fp32


def test_a_tensor_stays_where_it_is_and_device_is_not_consulted():
    x = torch.tensor(PTS, dtype=F64, requires_grad=True)
    t = _inputs.to_device(x, "no such device")
    assert t.data_ptr() == x.data_ptr() and not t.requires_grad               # detached, not copied
    with pytest.raises(RuntimeError):
        _inputs.to_device(PTS, "no such device")                                # anything else does go to `device`


def test_kept_dtypes_stay_and_others_become_the_last_kept():
    both = (F32, F64)
    for src, keep, want in ((F32, (F32,), F32), (F64, (F32,), F32), (torch.int64, (F32,), F32), (torch.float16, (F32,), F32),
                            (F32, both, F32), (F64, both, F64), (torch.int64, both, F64), (torch.float16, both, F64)):
        x = torch.tensor(PTS).to(src)
        assert _inputs.points(x, "cpu", "tag", keep).dtype == want, (src, keep)
        assert _inputs.points(x.numpy(), "cpu", "tag", keep).dtype == want, (src, keep)
    assert _inputs.to_device(torch.tensor(PTS, dtype=F32), "cpu", F64).dtype == F64             # the fp64 form widens
    assert _inputs.to_device(torch.tensor([1, 2], dtype=torch.uint8), "cpu", F64, keep=(torch.uint8, F32)).dtype == torch.uint8


def test_a_non_contiguous_tensor_comes_back_contiguous():
    x = torch.arange(12, dtype=F32).reshape(3, 4).T                            # (4, 3), strides (1, 4)
    assert not x.is_contiguous()
    for t in (_inputs.to_device(x, "cpu", F32), _inputs.points(x, "cpu", "tag"), _inputs.to_device(x, "cpu")):
        assert t.is_contiguous() and torch.equal(t.to(F32), x)
    assert _inputs.to_device(np.arange(12.0).reshape(3, 4).T, "cpu").is_contiguous()


@pytest.mark.parametrize("bad", [np.zeros((4, 2)), np.zeros(3), np.zeros((2, 3, 3)), torch.zeros(3, 4)])
def test_wrong_point_shapes_carry_the_callers_tag(bad):
    with pytest.raises(ValueError, match=r"^some_caller: points must be \(n, 3\), got \("):
        _inputs.points(bad, "cpu", "some_caller")


def test_edge_maps_shapes():
    m = torch.zeros(2, 5, 7)
    assert _inputs.edge_maps(m, 5, 7, "x: maps") is m and _inputs.edge_maps(m[..., None], 5, 7, "x: maps").shape == (2, 5, 7)
    assert _inputs.edge_maps(m[:0], 5, 7, "x: maps").shape == (0, 5, 7)
    for bad in (m, m[..., None]):                                               # h and w swapped
        with pytest.raises(ValueError, match=r"^x: maps must be \(F, 7, 5\) or \(F, 7, 5, 1\), got \(2, 5, 7"):
            _inputs.edge_maps(bad, 7, 5, "x: maps")
    for bad in (m[0], m[..., None].expand(2, 5, 7, 3), m[:, None]):
        with pytest.raises(ValueError, match="x: maps must be"):
            _inputs.edge_maps(bad, 5, 7, "x: maps")
    with pytest.raises(ValueError, match=r"x: maps must be \(F, 5, 7\) or \(F, 5, 7, 1\) with F > 0, got \(0, 5, 7\)"):
        _inputs.edge_maps(m[:0], 5, 7, "x: maps", nonempty=True)


def test_host64():
    a = _inputs.host64(torch.tensor([[1, 2], [3, 4]], dtype=torch.int32, requires_grad=False))
    assert a.dtype == np.float64 and a.tolist() == [[1.0, 2.0], [3.0, 4.0]]
    assert _inputs.host64(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]
    assert _inputs.host64([[1, 2]]).dtype == np.float64 and _inputs.host64(np.float32(0.1)) == np.float64(np.float32(0.1))


def test_world_to_camera_is_one_inverse_per_matrix_bit_for_bit():
    c, s = np.cos(0.3), np.sin(0.3)
    pose_a = np.array([[c, -s, 0.0, 0.1], [s, c, 0.0, -2.0], [0.0, 0.0, 1.0, 3.5], [0.0, 0.0, 0.0, 1.0]])
    pose_b = np.array([[0.9, 0.1, -0.3, 1.0], [0.2, 1.1, 0.05, 0.25], [-0.1, 0.3, 0.8, -4.0], [0.0, 0.0, 0.0, 1.0]])
    k_a = np.array([[500.0, 0.0, 320.5], [0.0, 510.0, 240.25], [0.0, 0.0, 1.0]])
    k_b = np.eye(4)
    k_b[:3, :3] = [[300.0, 0.5, 100.0], [0.0, 310.0, 90.0], [0.0, 0.0, 1.0]]
    K, R, T = _inputs.world_to_camera([k_a, torch.as_tensor(k_b)], [torch.as_tensor(pose_a), pose_b.tolist()])
    assert all(a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] for a in (K, R, T)) and (K.shape, R.shape, T.shape) == ((2, 3, 3), (2, 3, 3), (2, 3))
    for i, (k, pose) in enumerate(((k_a, pose_a), (k_b, pose_b))):
        inv = np.linalg.inv(pose)
        assert np.array_equal(K[i], k[:3, :3]) and np.array_equal(R[i], inv[:3, :3]) and np.array_equal(T[i], inv[:3, 3])
    with pytest.raises(np.linalg.LinAlgError):
        _inputs.world_to_camera([k_a], [np.zeros((4, 4))])


def test_load_edge_dict(tmp_path):
    d = {"curves_ctl_pts": [[0.0] * 12], "lines_end_pts": [[0.0, 0.0, 0.0, 1.0, 0.0, 0.0]]}
    path = tmp_path / "parametric_edges.json"
    path.write_text(json.dumps(d))
    assert _inputs.load_edge_dict(d) is d
    assert isinstance(path, pathlib.Path) and _inputs.load_edge_dict(path) == d and _inputs.load_edge_dict(str(path)) == d
    with pytest.raises(FileNotFoundError):
        _inputs.load_edge_dict(str(tmp_path / "missing.json"))
