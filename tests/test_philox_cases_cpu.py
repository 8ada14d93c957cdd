"""No GPU: tests/philox_cases.py (the expected draws of the in-kernel sampler, per optimizer) is consistent with what include/ctk_hip.h
documents, never uses a Philox counter twice, and the oracle's float32 Box-Muller is close enough to the float64 transform that its
rounding cannot decide a J / u comparison of tests/test_gpu_device_rng.py."""
import numpy as np
import pytest

from oracle import ctk_oracle as O
import philox_cases as PC
from gmm_oracle import UNIFORM_STREAM, device_draws, pack_draws

# one configuration per optimizer: C = 2 and 3, P*C and H*C not multiples of 4, RPGD resampling every second step
CFGS = [("mppi", dict(N=13, H=35, C=1, P=5)), ("mppi", dict(N=9, H=7, C=3, P=7, offset=77)), ("cem", dict(N=21, H=7, C=2, its=3)),
        ("cem_naive_grad", dict(N=10, H=9, C=1, its=2)), ("random_action", dict(N=65, H=7, C=3)),
        ("rpgd", dict(N=48, H=12, C=1, P=4, k=8, resamp_per=2)), ("rpgd", dict(N=17, H=9, C=3, P=4, k=5, resamp_per=2, kind="normal")),
        ("gradient", dict(N=12, H=6, C=2)), ("cem_grad_bharadhwaj", dict(N=32, H=10, C=1, K=8, its=2)),
        ("cem_gmm", dict(N=30, H=5, C=2, its=2))]


@pytest.mark.parametrize("opt,cfg", CFGS)
def test_sizes_are_the_documented_ones(opt, cfg):
    for phase in ("reset", "step"):
        got = PC.expected_samples(opt, cfg, PC.SEED, 3, phase)
        assert got.dtype == np.float32 and got.size == PC.samples_documented(opt, cfg, phase), (opt, phase)
    assert set(o for o, _ in CFGS) == set(PC.OPTIMIZERS)


def test_layouts_against_the_existing_statements():
    """CEM-GMM: the same array as tests/gmm_oracle.py builds; MPPI with an offset: rows of the global population; bharadhwaj:
    elites on rows [0, K), the rest on rows K.. of stream `it`; gradient: word c of block 0"""
    assert PC.GMM_UNIFORM_STREAM == UNIFORM_STREAM
    g = dict(N=30, H=5, C=2, its=2)
    np.testing.assert_array_equal(PC.expected_samples("cem_gmm", g, 11, 4), pack_draws(*device_draws(11, 4, 2, 30, 10)))
    m = dict(N=9, H=7, C=3, P=7, offset=77)
    np.testing.assert_array_equal(PC.expected_samples("mppi", m, 5, 2).reshape(9, 21), O.device_noise(5, 0, 2, 0, 86, 21, "normal")[77:])
    b = dict(N=32, H=10, C=1, K=8, its=2)
    x = PC.expected_samples("cem_grad_bharadhwaj", b, 5, 1)
    np.testing.assert_array_equal(x[:80].reshape(8, 10), O.device_noise(5, 0, 1, 0, 32, 10, "normal")[:8])
    np.testing.assert_array_equal(x[80 + 240:].reshape(24, 10), O.device_noise(5, 1, 1, 0, 32, 10, "normal")[8:])
    t = PC.expected_samples("gradient", dict(N=12, H=6, C=2), 5, 3).reshape(12, 2)
    np.testing.assert_array_equal(t, O.device_noise(5, 0, 3, 0, 12, 4, "uniform")[:, :2])


@pytest.mark.parametrize("opt,cfg", CFGS)
def test_no_counter_is_used_twice(opt, cfg):
    """reset + 3 steps of the optimizer's schedule: every (row, block, call, stream) at most once — CEM-GMM's uniform streams
    0x40000000 + it against the normal streams `it` included"""
    used = [PC.counters(opt, cfg, pos, phase) for phase, pos, draws in PC.schedule(opt, cfg, 3) if draws]
    allc = np.concatenate(used)
    assert len(allc) > 0 and len(np.unique(allc, axis=0)) == len(allc)
    sched = PC.schedule(opt, cfg, 3)
    assert [p for _, p, _ in sched] == list(range(len(sched)))           # the position moves by one per reset-that-draws and per step
    if opt == "rpgd":
        assert [d for _, _, d in sched] == [True, True, False, True]     # resamp_per = 2: steps 0 and 2 resample, step 1 still moves it


# Box-Muller in float32 against float64 on the same words.  Each of log, sqrt, the product 2*pi*u2 (kept), cos / sin and the final
# product rounds once (NumPy's float32 log / sin / cos are within ~1 ulp): a few ulp of a value of magnitude up to
# sqrt(-2 ln 2^-24) = 5.8, where one ulp is 4.8e-7 ([4, 8)).  Recorded here: 3.4e-7 absolute / 2.4e-7 relative over the 51 200 draws of
# the headline shape; the bound is 2 ulp at the largest magnitude.
NORMAL_ABS = 2 * 4.77e-7


@pytest.mark.parametrize("N,cols,call,stream", [(1024, 50, 0, 0), (1024, 50, 7, 2), (130, 5, 1, 0), (1024, 30, 3, 1)])
def test_float32_box_muller_close_to_float64(N, cols, call, stream):
    f32n = O.device_noise(PC.SEED, stream, call, 0, N, cols, "normal").astype(np.float64)
    f64n = PC.normal_f64(PC.SEED, stream, call, 0, N, cols)
    err = np.abs(f32n - f64n)
    big = np.abs(f64n) > 1e-2
    print(f"N*cols {N * cols}: max abs {err.max():.2e}, max rel (|x| > 1e-2) {np.max(err[big] / np.abs(f64n[big])):.2e}")
    assert err.max() <= NORMAL_ABS
    assert abs(f64n.mean()) < 5 / np.sqrt(f64n.size) and abs(f64n.std() - 1) < 5 / np.sqrt(2 * f64n.size)     # it IS a standard normal
    assert PC.small_u1(PC.SEED, stream, call, 0, N, cols).sum() > 0 if N * cols > 20000 else True


@pytest.mark.parametrize("N,H,p,off", PC.MPPI_ODE_SHAPES)
def test_box_muller_rounding_cannot_decide_mppi_costs(N, H, p, off):
    """J of the oracle fed the float32 draws against J fed the float64 transform: at most 1/5 of the J tolerance"""
    J = []
    for draws in ("f32", "f64"):
        pred = O.Predictor("ODE", dt=0.02, env=O.EnvParams(terminal_weight=0.3, target_position=0.05))
        o = O.MPPI(pred, O.Cost(pred.env), num_rollouts=N, mpc_horizon=H, period_interpolation_inducing_points=p)
        z = (PC.expected_samples("mppi", dict(N=N, H=H, C=1, P=o.P, offset=off), PC.SEED, 0) if draws == "f32"
             else PC.normal_f64(PC.SEED, 0, 0, off, N, o.P).astype(np.float32))
        o.step(PC.S0, z.reshape(N, o.P, 1))
        J.append(o.J.astype(np.float64))
    rel = np.max(np.abs(J[0] - J[1]) / np.abs(J[1]))
    print(f"MPPI N{N} H{H}: J moves by {rel:.2e} relative")
    assert rel <= PC.J_RTOL / 5


@pytest.mark.parametrize("N,H,K,its", PC.CEM_ODE_SHAPES)
def test_box_muller_rounding_cannot_decide_cem_costs(N, H, K, its):
    J = []
    for draws in ("f32", "f64"):
        pred = O.Predictor("ODE", dt=0.02, env=O.EnvParams(terminal_weight=0.2))
        o = O.CEM(pred, O.Cost(pred.env), num_rollouts=N, mpc_horizon=H, cem_outer_it=its, cem_best_k=K)
        z = (O.device_noise(PC.SEED, 0, 0, 0, N, H, "normal") if draws == "f32" else PC.normal_f64(PC.SEED, 0, 0, 0, N, H).astype(np.float32))
        J.append(o.update_distribution(np.tile(PC.S0.reshape(1, 4), (N, 1)), z.reshape(N, H, 1))[2].astype(np.float64))
    rel = np.max(np.abs(J[0] - J[1]) / np.abs(J[1]))
    print(f"CEM N{N} H{H}: J of the first iteration moves by {rel:.2e} relative")
    assert rel <= PC.J_RTOL / 5
