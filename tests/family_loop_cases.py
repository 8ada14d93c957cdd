"""Cases of the closed loops of the CEM and RPGD batches on the device (BatchClosedLoop(cem_batch) / BatchClosedLoop(rpgd_batch);
include/ctk_hip_loop.h), shared by test_family_loop_cpu.py and test_gpu_family_loop.py.  A plain module, not a conftest.

Start states, plant overrides, sub-step counts, sigmas, noise seeds and every bound are batch_run_cases.py's and batch_episode_cases.py's
(B 3, 5 where a split into launches is wanted; runs of 6 steps, 10 where segments are wanted): they are used, not restated.  The
controller sizes are the smallest at which each kernel branch is taken, from the CONFIGS of test_gpu_cem_batch.py and
test_gpu_rpgd_batch.py; one case per family has a warm-up step of 3 iterations, so that a run of 6 steps crosses the first-step rule of
the iteration count, and the RPGD cases resample every 1, 2 or 3 steps, so that it crosses at least two resampling steps.

The counter rules of a segment's step records are restated here on the host (cem_counters, rpgd_counters): what step t of a run must
carry, given the problem's counters at the start of the run."""
import batch_run_cases as K

CEM_CASES = ("one_workgroup", "quad2d", "hover")
RPGD_CASES = ("cartpole_small", "cartpole_partial", "cartpole_full_wave", "quad2d", "hover")
WARMUP = dict(warmup=True, warmup_iterations=3)               # of one_workgroup and cartpole_small
FAMILY_CASES = [("cem", c) for c in CEM_CASES] + [("rpgd", c) for c in RPGD_CASES]
PREFIX = {"cem": "ctk_cem_batch", "rpgd": "ctk_rpgd_batch"}
BUFFERS = {"cem": ("U_NOM", "STD", "J", "Q", "BEST_IDX"),
           "rpgd": ("Q", "J", "U_NOM", "PLAN", "ADAM_M", "ADAM_V", "AGES", "BEST_IDX")}
# the fourteen entries every family has for its closed loop: ctk_hip_run.h's five and ctk_hip_episode.h's nine
ENTRIES = ("plant_set_param", "plant_get_param", "plant_clear_params", "plant_step", "run",
           "plant_set_noise", "plant_get_noise", "plant_clear_noise", "plant_set_noise_seed", "plant_get_noise_seed",
           "plant_noise_get_position", "plant_noise_set_position", "plant_step_noisy", "episodes")
CEM_SPLIT_SWITCH = "CTK_CEM_BATCH_MAX_PROBLEMS_PER_LAUNCH"     # K.SPLIT_PER_LAUNCH: 5 problems as 2 + 2 + 1 launches
SEGMENT_SWITCH = "CTK_BATCH_RUN_SEGMENT_STEPS"                # K.SEGMENT_STEPS: 10 steps as 4 + 4 + 2


def batch_kwargs(family, case):
    """the keywords of CtkCemBatch / CtkRpgdBatch for a case (the test modules are imported here: they need the built library)"""
    if family == "cem":
        import test_gpu_cem_batch as TC
        kw = TC.common_kw(case, False)
        if case == "one_workgroup":
            kw.update(WARMUP)
        return kw
    import test_gpu_rpgd_batch as TR
    kw = dict(TR.CONFIGS[case]())
    if case == "cartpole_small":
        kw.update(WARMUP)
    return kw


def environment(family, case):
    return {"one_workgroup": "CartPole", "quad2d": "Quad2D", "hover": "Hover"}.get(case, "CartPole")


def cem_counters(count, tag, steps, *, warmup, warmup_iterations, cem_outer_it):
    """[(its, tag0)] of the next `steps` steps of a CEM problem that has taken `count` steps since its creation or reset and whose next
    unused hand-off tag is `tag`, and the tag after them.  A step whose tags would wrap past 2^32 restarts at 1: tag 0 is never used."""
    out = []
    for t in range(steps):
        its = warmup_iterations if (warmup and count + t == 0) else cem_outer_it
        if tag + its >= 2 ** 32:
            tag = 1
        out.append((its, tag))
        tag = (tag + its) % 2 ** 32
    return out, tag


def rpgd_counters(count, adam_step, steps, *, warmup, warmup_iterations, outer_its, resamp_per):
    """[(iters, t0, resample)] of the next `steps` steps of an RPGD problem that has taken `count` steps since its reset and `adam_step`
    Adam iterations"""
    out = []
    for t in range(steps):
        iters = (warmup_iterations if warmup else outer_its) if count + t == 0 else outer_its
        out.append((iters, adam_step, 1 if (count + t) % resamp_per == 0 else 0))
        adam_step += iters
    return out

