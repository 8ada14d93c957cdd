"""-m gpu: CEM, random-action and CEM + naive gradient through the C ABI against fixtures RECORDED FROM THE UNMODIFIED REFERENCE
modules (optimizer_cem_tf.py, optimizer_random_action_tf.py, optimizer_cem_naive_grad_tf.py; tests/golden/make_golden.py:
record_tf_only_optimizers — their `tf.*` calls served by the torch-backed stand-in under tests/golden/standins/tensorflow).

CEM runs in BOTH device forms: the one-launch step (ctk_cem_fused.hip) and the launch-per-phase form (CTK_NO_CEM_FUSED).

What "equal" means where a sort decides: two fp32 evaluations of the same costs may order differently the plans whose costs lie
closer than the cost tolerance.  The tests therefore (i) require the device's elite set to differ from the reference's only in
members within `J_RTOL` of the cut, (ii) hold `u` / mean / stdev to the tight tolerance whenever the sets are the same (every
fixture but the full-size cfg3, where the cut falls between costs 1e-6 apart), and to the bound a swapped member implies
otherwise.  Observed margins are appended to profiles/r04_parity_margins.txt by tests/margins.py."""
import numpy as np
import pytest

from control_toolkit_amd import CtkEngine
from helpers import load, env_from, CEM_CASES, RANDOM_CASES, CEM_NAIVE_GRAD_CASES
from margins import record

pytestmark = pytest.mark.gpu

J_RTOL = 1e-5          # observed worst 1.3e-6 (profiles/r04_parity_margins.txt); SURVEY 8c proposes 1e-5
Q_TOL = dict(rtol=1e-5, atol=2e-6)
TRAJ_TOL = dict(rtol=1e-4, atol=4e-5)


def engine_from(d, opt, **kw):
    pred, envname = str(d["predictor"]), str(d["environment"])
    e = CtkEngine(opt, pred, environment=envname, num_rollouts=int(d["num_rollouts"]), mpc_horizon=int(d["mpc_horizon"]), dt=float(d["dt"]),
                  action_low=d["low"], action_high=d["high"], **kw)
    env = env_from(d)
    for n in env.param_names():
        e.set_param(n, float(getattr(env, n)))
    if pred == "MLP":
        e.set_predictor_weights(d["mlp_weights"])
    return e


def elite_sets_agree(J_ref, best_dev, K, rtol):
    """the device's elite set vs the reference's: members may differ only where the reference's own cost is within rtol of the cut;
    returns the number of members that differ"""
    ref_sorted = np.argsort(J_ref, kind="stable")
    ref_set, dev_set = set(ref_sorted[:K].tolist()), set(np.asarray(best_dev).tolist())
    assert len(dev_set) == K
    cut = 0.5 * (J_ref[ref_sorted[K - 1]] + J_ref[ref_sorted[min(K, len(J_ref) - 1)]])
    for i in ref_set ^ dev_set:
        assert abs(J_ref[i] - cut) <= rtol * abs(cut), (i, J_ref[i], cut)
    return len(ref_set - dev_set)


@pytest.mark.parametrize("form", ["one_launch", "launch_per_phase"])
@pytest.mark.parametrize("case", CEM_CASES)
def test_cem_matches_reference_golden(monkeypatch, case, form):
    d = load(f"cem_{case}.npz")
    N, H, K, C = int(d["num_rollouts"]), int(d["mpc_horizon"]), int(d["cem_best_k"]), len(d["low"])
    if form == "launch_per_phase":
        monkeypatch.setenv("CTK_NO_CEM_FUSED", "1")
    e = engine_from(d, "cem", cem_outer_it=int(d["cem_outer_it"]), cem_best_k=K,
                    cem_initial_action_stdev=float(d["cem_initial_action_stdev"]), cem_stdev_min=float(d["cem_stdev_min"]),
                    warmup=int(bool(d["warmup"])), warmup_iterations=int(d["warmup_iterations"]), materialize_trajectories=f"traj_0" in d.files)
    monkeypatch.delenv("CTK_NO_CEM_FUSED", raising=False)
    if str(d["environment"]) == "CartPole" and str(d["predictor"]) == "ODE":
        assert e.dominant_kernel().startswith("ctk_cem_fused") == (form == "one_launch"), e.dominant_kernel()
    np.testing.assert_array_equal(e.read("U_NOM"), d["dist_mue_init"])
    np.testing.assert_array_equal(e.read("STD"), d["stdev_init"])
    span = float(np.max(d["high"] - d["low"]))
    for t in range(int(d["steps"])):
        noise = d[f"noise_{t}"]
        assert e.samples_needed() == noise.size                         # warm-up switch (optimizer_cem_tf.py:92)
        u = e.step(d[f"s_{t}"], noise, u_prev=d[f"u_prev_{t}"])
        Jg, Jr = e.read("J"), d[f"J_{t}"]
        tag = f"cem_{case}[{form}] step {t}"
        record(tag, "Q", e.read("Q"), d[f"Q_{t}"], **Q_TOL)
        record(tag, "J", Jg, Jr, rtol=J_RTOL)
        # Q of the last iteration = mu + noise * std of the one before: every earlier refit is inside this comparison
        np.testing.assert_allclose(e.read("Q"), d[f"Q_{t}"], **Q_TOL)
        np.testing.assert_allclose(Jg, Jr, rtol=J_RTOL)
        if f"traj_{t}" in d.files:
            record(tag, "traj", e.read("TRAJ"), d[f"traj_{t}"], **TRAJ_TOL)
            np.testing.assert_allclose(e.read("TRAJ"), d[f"traj_{t}"], **TRAJ_TOL)
        bg = e.read("BEST_IDX")
        swapped = elite_sets_agree(Jr, bg, K, J_RTOL)
        assert np.all(np.diff(Jg[bg]) >= 0) and bg[0] == np.argmin(Jg)   # ascending by the device's own costs (tf.argsort)
        # a swapped member moves the mean by at most span / K and the variance accordingly
        slack = swapped * span / K
        record(tag, "dist_mue", e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6 + slack)
        record(tag, "stdev", e.read("STD"), d[f"stdev_{t}"], rtol=5e-5, atol=2e-6 + slack)
        np.testing.assert_allclose(e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=2e-6 + slack)
        np.testing.assert_allclose(e.read("STD"), d[f"stdev_{t}"], rtol=5e-5, atol=2e-6 + slack)
        if Jr[np.argsort(Jr)[1]] - Jr.min() > J_RTOL * abs(Jr.min()):    # u = the best plan's first input (:101)
            record(tag, "u", u, d[f"u_{t}"], rtol=1e-5, atol=2e-6)
            np.testing.assert_allclose(u, d[f"u_{t}"], rtol=1e-5, atol=2e-6)
        # the recorded closed loop continues from the reference's own distribution
        e.set_state(np.concatenate([d[f"dist_mue_{t}"].reshape(H * C), d[f"stdev_{t}"].reshape(H * C), d[f"u_{t}"].reshape(C), [t + 1]]).astype(np.float32))
    e.close()


@pytest.mark.parametrize("case", RANDOM_CASES)
def test_random_action_matches_reference_golden(case):
    """`cfg1` is BASELINE configs[0] (N 32, H 10) on the HIP path"""
    d = load(f"random_{case}.npz")
    e = engine_from(d, "random_action", materialize_trajectories=True)
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"u01_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"random_{case} step {t}"
        record(tag, "Q", e.read("Q"), d[f"Q_{t}"], rtol=1e-6, atol=1e-7)
        record(tag, "J", e.read("J"), d[f"J_{t}"], rtol=J_RTOL)
        record(tag, "traj", e.read("TRAJ"), d[f"traj_{t}"], **TRAJ_TOL)
        np.testing.assert_allclose(e.read("Q"), d[f"Q_{t}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(e.read("J"), d[f"J_{t}"], rtol=J_RTOL)
        np.testing.assert_allclose(e.read("TRAJ"), d[f"traj_{t}"], **TRAJ_TOL)
        Jr = d[f"J_{t}"]
        assert Jr[np.argsort(Jr)[1]] - Jr.min() > J_RTOL * abs(Jr.min())           # fixtures with a clear winner
        assert int(e.read("BEST_IDX")[0]) == int(np.argmin(Jr))
        np.testing.assert_allclose(u, d[f"u_{t}"], rtol=1e-6, atol=1e-7)             # u = Q[best, 0, :] (:68)
        e.set_state(d[f"u_{t}"].astype(np.float32))
    e.close()


def test_random_action_three_launch_step_equals_one_launch_step(monkeypatch):
    """CartPole through rollout + ctk_select_topk + ctk_g_pick_best_first: a handle created without the hand-off words (CTK_NO_LL,
    read at ctk_create) has no in-launch arg-min.  Same rollouts, same total order (J, index), same plan read back: u and the
    winner's index equal the default handle's bit for bit."""
    d = load("random_cfg1.npz")
    assert str(d["environment"]) == "CartPole" and str(d["predictor"]) == "ODE"
    one = engine_from(d, "random_action")
    monkeypatch.setenv("CTK_NO_LL", "1")
    three = engine_from(d, "random_action")
    monkeypatch.delenv("CTK_NO_LL")
    for t in range(int(d["steps"])):
        u1 = one.step(d[f"s_{t}"], d[f"u01_{t}"], u_prev=d[f"u_prev_{t}"])
        u3 = three.step(d[f"s_{t}"], d[f"u01_{t}"], u_prev=d[f"u_prev_{t}"])
        np.testing.assert_array_equal(np.asarray(u3, np.float32).view(np.uint32), np.asarray(u1, np.float32).view(np.uint32))
        assert int(three.read("BEST_IDX")[0]) == int(one.read("BEST_IDX")[0]) == int(np.argmin(d[f"J_{t}"]))
        np.testing.assert_allclose(u3, d[f"u_{t}"], rtol=1e-6, atol=1e-7)
        for e in (one, three):
            e.set_state(d[f"u_{t}"].astype(np.float32))
    one.close()
    three.close()


@pytest.mark.parametrize("case", CEM_NAIVE_GRAD_CASES)
def test_cem_naive_grad_matches_reference_golden(case):
    d = load(f"cem_naive_grad_{case}.npz")
    H, K, C = int(d["mpc_horizon"]), int(d["cem_best_k"]), len(d["low"])
    e = engine_from(d, "cem_naive_grad", cem_outer_it=int(d["cem_outer_it"]), cem_best_k=K, cem_initial_action_stdev=float(d["cem_initial_action_stdev"]),
                    cem_stdev_min=float(d["cem_stdev_min"]), learning_rate=float(d["learning_rate"]), gradmax_clip=float(d["gradmax_clip"]))
    span = float(np.max(d["high"] - d["low"]))
    for t in range(int(d["steps"])):
        u = e.step(d[f"s_{t}"], d[f"noise_{t}"], u_prev=d[f"u_prev_{t}"])
        tag = f"cem_naive_grad_{case} step {t}"
        # Q moved by lr * clipped gradient (|g| <= gradmax_clip = 10); observed worst 6.6e-6 absolute on Q, 1.6e-6 on the mean
        record(tag, "Q", e.read("Q"), d[f"Q_{t}"], rtol=2e-5, atol=2e-5)
        record(tag, "J", e.read("J"), d[f"J_{t}"], rtol=J_RTOL)
        np.testing.assert_allclose(e.read("Q"), d[f"Q_{t}"], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(e.read("J"), d[f"J_{t}"], rtol=J_RTOL)
        swapped = elite_sets_agree(d[f"J_{t}"], e.read("BEST_IDX"), K, J_RTOL)
        slack = swapped * span / K
        record(tag, "dist_mue", e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=1e-5 + slack)
        record(tag, "stdev", e.read("STD"), d[f"stdev_{t}"], rtol=1e-4, atol=1e-5 + slack)
        record(tag, "u", u, d[f"u_{t}"], rtol=1e-5, atol=1e-5 + slack)
        np.testing.assert_allclose(e.read("U_NOM"), d[f"dist_mue_{t}"], rtol=1e-5, atol=1e-5 + slack)
        np.testing.assert_allclose(e.read("STD"), d[f"stdev_{t}"], rtol=1e-4, atol=1e-5 + slack)
        np.testing.assert_allclose(u, d[f"u_{t}"], rtol=1e-5, atol=1e-5 + slack)     # u = the refitted MEAN's first input (:103)
        e.set_state(np.concatenate([d[f"dist_mue_{t}"].reshape(H * C), d[f"stdev_{t}"].reshape(H * C), d[f"u_{t}"].reshape(C), [t + 1]]).astype(np.float32))
    e.close()
