"""Host side of the LBA step (no GPU): misc.get_twin_rel_pose against the unmodified reference's recording
(tests/golden/lba_step.npz, tools/gen_lba_step_golden.py), the fixture's input checksums against the shared input helper, the
driver's trajectory helpers, and the float64 restatement's verdict on the convergence condition the GPU test relies on."""
import os

import numpy as np
import pytest
import torch

import lba_fp64 as lf
import lba_step_inputs as li
from conftest import GOLDEN
from neuralrgbd_amd import lba_step, misc


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "lba_step.npz")))


def test_fixture_inputs_match_the_helper(golden):
    sc = li.scene()
    for k, v in li.checksums(sc).items():
        assert float(golden[k]) == v, k
    assert (int(golden["H"]), int(golden["W"]), int(golden["D"]), int(golden["seed"])) == (li.H, li.W, li.D, li.SEED)
    assert int(golden["max_iter"]) == li.MAX_ITER and float(golden["step"]) == li.LBA_STEP


def test_get_twin_rel_pose_equals_the_reference_exactly(golden):
    traj, dso, dataset = li.index_traj()
    cases = li.twin_cases()
    assert int(golden["twin_n"]) == len(cases)
    for n, (ref_indx, t_win_r, step, kw) in enumerate(cases):
        kw = dict(kw)
        if kw.pop("with_dso", False):
            kw["traj_extMs_dso"] = [d.copy() for d in dso]
        poses, idx = misc.get_twin_rel_pose([t.copy() for t in traj], ref_indx, t_win_r, step, dataset=dataset, **kw)
        assert list(idx) == golden["twin_%03d_idx" % n].tolist(), (n, kw)
        got = np.stack([p.numpy() for p in poses])
        assert got.dtype == np.float32 and np.array_equal(got, golden["twin_%03d_poses" % n]), (n, kw)


def test_last_frame_takes_its_neighbours_pose():
    traj, _, _ = li.index_traj()
    poses, idx = misc.get_twin_rel_pose(traj, 15, 2, 5)
    assert idx == [5, 10, 20, 25]
    from neuralrgbd_amd import homography
    assert np.array_equal(poses[-1].numpy(), homography.get_rel_extrinsicM(traj[15], traj[24]).astype(np.float32))
    assert not np.array_equal(poses[-1].numpy(), homography.get_rel_extrinsicM(traj[15], traj[25]).astype(np.float32))
    poses, idx = misc.get_twin_rel_pose(traj, 15, 2, 5, opt_next_frame=True)
    assert idx == [5, 10, 16, 20, 25] and len(poses) == 5
    with pytest.raises(AssertionError):
        misc.get_twin_rel_pose(traj, 15, 2, 5, use_dso_R=True)


def test_trajectory_helpers():
    traj, _, _ = li.index_traj(12)
    assert lba_step.valid_poses(traj, [0, 3, 5])
    traj[3] = np.eye(4)
    assert not lba_step.valid_pose(traj[3]) and not lba_step.valid_poses(traj, [0, 3]) and lba_step.valid_poses(traj, [0, 4])
    bad = traj[4].copy(); bad[0, 0] = np.nan
    assert not lba_step.valid_pose(bad)
    tn = lba_step.get_t_norms(traj, 1)
    valid = [t for t in traj[1:] if lba_step.valid_pose(t)]
    assert len(tn) == len(valid) - 2
    assert tn[0] == np.linalg.norm(valid[2][:3, 3] - valid[0][:3, 3])
    cp = lba_step.copy_list(traj)
    lba_step.rescale_traj_t(cp, 2.0)
    assert np.array_equal(cp[5][:3, 3], 2.0 * traj[5][:3, 3]) and np.array_equal(cp[5][:3, :3], traj[5][:3, :3])
    assert lba_step.window_indices(10, 2, 5) == [0, 5, 15, 20] and lba_step.window_indices(2, 2, 1) == [0, 1, 3, 4]


def test_fp64_restatement_satisfies_the_convergence_condition():
    """The GPU test asserts that every source pose of the first-window optimisation ends closer to the truth than it started.
    That is a property of the input (seed, perturbation, iterations, step), checked here on the float64 restatement of the
    optimiser with float64 maps, so the GPU assertion does not rest on what the GPU path itself returns."""
    sc = li.scene()
    BV = sc["BV"][0].double()
    d = torch.from_numpy(li.D_CANDI).view(-1, 1, 1)
    dmap, conf = (BV.exp() * d).sum(0), BV.max(0)[0].exp() ** 2
    traj = [t.copy() for t in sc["traj"]]
    inits, idx = misc.get_twin_rel_pose(traj, li.REF, li.T_WIN_R * li.STEP, 1, dataset=sc["frames"])
    e0 = li.rel_errors(traj, sc["true"], li.REF, idx)
    levels = lf.level_inputs(sc["frames"][li.REF]["img"], [sc["frames"][i]["img"] for i in idx], dmap[None, None],
                             conf[None, None], li.cams(), li.DW_SCALES)
    uq0 = torch.stack([misc.Rotation2UnitQ(p[:3, :3].clone()) for p in inits])
    t0 = torch.stack([p[:3, 3] for p in inits])
    r = lf.run(levels, uq0, t0, li.MAX_ITER, li.LBA_STEP, [1, 1], joint=False)
    P = lf.uq_to_pose(r["uq"], r["t"])
    for k, i in enumerate(idx):
        traj[i] = P[k] @ traj[li.REF]
    e1 = li.rel_errors(traj, sc["true"], li.REF, idx)
    for a, b in zip(e0, e1):
        assert b[0] < a[0] and b[1] < a[1], (e0, e1)
