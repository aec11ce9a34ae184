"""Hidden widths off the 4-grid and batches under one 16-row tile on the device, against the oracle.

A hidden width is the row stride of every activation and delta buffer and of the next layer's W_ext, so a
width that is no multiple of 4 turns off every 16-B operand path: add_gemm's float4 gates (k_gemm's
element-wise load_a / load_b, a per-problem g.vec == 0 inside a VEC launch), k_dwl's dword staging
(dwl_issue<false>), the dX launches' unaligned W_ext rows, the row kernels on a row that is no whole number
of float4s, the bf16 pair layout with a half-filled last pair.  A batch below 16 rows leaves every tile, every
k_fwd2 block and every rows-per-workgroup kernel partly filled.  The bodies and the bars are those of
test_gpu_depth.py / test_gpu_engine.py / test_gpu_wide.py / test_gpu_dw.py / test_gpu_bf16.py, called as they
are with the ragged shapes entered into their tables; no bar is widened.  B = 64, S = 17, A = 6, N = 2,000,
random normalisers unless a case says otherwise.

Which plan a handle takes (printed by the one-update body, asserted in test_plans_of_the_ragged_handles):
two hidden layers per net run build_plan whatever the widths (q.head+critic.bwd1 and pi.q.head+pi.q.bwd1, the
linearity launches, are always there), and its folds follow the shape.  (64, 64) takes the whole fused plan
at every batch from 1 to 64: actor.fwd01, q.fwd01+actor.head, critic.adam+actor.head, pi.q.fwd01,
actor.head.bwd+actor.bwd1.  off4 (the actor on the grid, the critics off it) keeps q.fwd0+actor.head and
actor.fwd01 but no critic pair and actor.head.bwd as its own launch; a32 (Aout = 32 > 16) keeps actor.fwd01
and actor.head / actor.head.bwd as launches; odd2, a31_odd, pss_odd, tiny23, ln_odd and the eo cases take
none of the folds: actor.fwd0, actor.fwd1, actor.head, q.fwd0, q.fwd1, ..., actor.head.bwd, actor.bwd1.
odd_mid3 (three layers), tiny1 (one) and odd_wide / ln_wide_odd (above 512) run the generic plan: no "+" in
any launch name.

The reference alone (test_premise_of_the_ragged_cases_on_the_cpu): the oracle in fp32 against itself in
fp64, make_learner(seed=3, N=2000) and the draws of test_one_update_any_depth, must stay inside a quarter
of each bar (5e-6 losses, 5e-5 gradients relative to the tensor's max) with every compared gradient tensor
non-zero.  Measured over the 13 cases and the 10 batch cases: losses 1.2e-7 .. 3.9e-7 (worst B = 1 on
(63, 65): 1.8e-6), gradients 1.8e-7 .. 1.1e-6 (worst tiny1: 3.9e-6), smallest max |g| 3.4e-2 .. 1.4 (worst
tiny1: 3.9e-3).  tanh / elu on the tiny cases: a relu layer 1 .. 3 wide can be dead at a seed.

On the device: every loss within 8e-7 and every actor gradient within 2e-6 (tiny1; 3e-7 elsewhere) of the
oracle, a tenth of the bars or less; the closing run's log is profiles/ragged_pytest_gpu_v1.log.
"""
import numpy as np
import pytest

import sac_oracle as O
import test_gpu_bf16 as BF
import test_gpu_depth as D
import test_gpu_dw as DW
import test_gpu_engine as E
import test_gpu_wide as W
from helpers import make_learner, make_pair, oracle_step, relerr

N = 2000
RAGGED = {
    # every stride = 1 or 3 (mod 4)
    "odd2": dict(hidden=(63, 65)),
    # strides = 2 (mod 4): 8-B but not 16-B rows; the actor on the grid, the critics off it
    "off4": dict(hidden=(64, 64), wm=dict(critic_hidden=(66, 62))),
    # an odd stride between two aligned layers: forward, dX and dW on both sides
    "odd_mid3": dict(hidden=(64, 61, 64)),
    # K = 1, N = 1: one-column tiles
    "tiny1": dict(hidden=(1,), act="tanh"),
    # K and ld below one float4
    "tiny23": dict(hidden=(2, 3), wm=dict(critic_hidden=(3, 1)), act="elu"),
    # both ends of the second 512-column slab, odd
    "odd_wide": dict(hidden=(513, 1023), wm=dict(critic_hidden=(1023, 513))),
    "ln_odd": dict(hidden=(67, 64), layer_norm=True),
    "ln_wide_odd": dict(hidden=(1021, 64), layer_norm=True),
    # Aout = 14 on an odd K
    "pss_odd": dict(S=9, A=7, hidden=(33, 47), per_state_std=True, act="elu"),
    # the head limit: one lane per action; ldS = 4 holding one column
    "a32": dict(S=1, A=32, hidden=(64, 64)),
    "a31_odd": dict(S=2, A=31, hidden=(63, 65)),
    # the expert term through odd world models
    "eo_odd": dict(use_expert=True, model_hidden=(65, 127), ne=12),
    "eo_srn_mixed": dict(use_expert=True, model_hidden=(64, 64), ne=12,
                         wm=dict(separate_reward_nn=True, reward_hidden=(7, 9), reward_act="tanh")),
}
# the batch cases' widths: the fused plan, and the same batches off the grid
GRID = {"grid2": dict(hidden=(64, 64))}
BATCHES = [(case, B) for case in ("grid2", "odd2") for B in (1, 2, 15, 16, 17)]
ALL = dict(RAGGED, **GRID)


def _enter(monkeypatch, case):
    monkeypatch.setitem(D.CASES, case, dict(ALL[case], N=N))


def _premise(case, B):
    """The oracle's one update of `case` in fp32 against fp64 (the learner and the draws of
    test_one_update_any_depth): (largest relative loss difference, largest gradient difference relative to
    the tensor's max, smallest max |g| of the compared reference gradients)."""
    kw = dict(ALL[case])
    kw.setdefault("ne", 12)
    kw.setdefault("act", "relu")
    out = []
    for dtype in (np.float64, np.float32):
        ocfg, st, buf, nrm, expert = make_learner(B=B, seed=3, N=N, normalizers="random", **kw)
        eo = expert is not None
        rs, gen = np.random.RandomState(17), np.random.default_rng(4)
        R = O.draw_step_randoms(rs, N, B, ocfg.A, n_expert=kw["ne"] if eo else 0, gen=gen, n_models=2)
        keep = {}
        ref = oracle_step(st.astype(dtype), ocfg, nrm, buf, R, expert, keep)
        grads = list(keep["q0_grads"]) + list(keep["q1_grads"])
        ga = list(keep["actor_grads"])
        grads += ga[:2] + ga[4:] if ocfg.layer_norm else ga        # the Dense layers, as the device test compares
        losses = [ref[k] for k in ("q1_loss", "q2_loss", "p_loss", "alpha_loss")] + ([ref["mse_loss"]] if eo else [])
        out.append((np.array(losses, np.float64), [np.asarray(g, np.float64) for g in grads]))
    (l64, g64), (l32, g32) = out
    return (float(np.max(np.abs(l32 - l64) / np.abs(l64))), max(relerr(a, b) for a, b in zip(g32, g64)),
            min(float(np.max(np.abs(g))) for g in g64))


@pytest.mark.parametrize("case,B", [(c, 64) for c in RAGGED] + BATCHES)
def test_premise_of_the_ragged_cases_on_the_cpu(case, B):
    """No device: the reference alone stays inside a quarter of the device test's bars at every ragged
    shape, and no compared gradient tensor is all zero (a dead layer would compare 0 with 0)."""
    loss, grad, gmin = _premise(case, B)
    print(f"premise {case} B={B}: loss {loss:.2e} (quarter bar 5e-6) gradient {grad:.2e} (5e-5) smallest max|g| {gmin:.2e}")
    assert loss < 5e-6, loss
    assert grad < 5e-5, grad
    assert gmin > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(RAGGED))
def test_one_update_ragged(gpu_available, monkeypatch, case):
    """One update vs the fp64 oracle: the four losses and the MSE term at 2e-5, the sampler's indices and
    the stream bit-exact, every Dense gradient through Adam's first moment at 2e-4 of the tensor's max,
    Polyak at 1e-5 (the body of test_one_update_any_depth)."""
    _enter(monkeypatch, case)
    D.test_one_update_any_depth(gpu_available, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case,B", BATCHES)
def test_one_update_small_batches(gpu_available, monkeypatch, case, B):
    """The same body at batches of 1, 2, 15, 16 and 17 rows, on (64, 64) (the fused plan) and (63, 65).
    At B = 1 every mean is over one row, the sampler draws one index and each noise draw is one row of A = 6
    normals; B = 15 and 17 leave an odd number of rows on either side of the 16-row tile."""
    _enter(monkeypatch, case)
    D.test_one_update_any_depth(gpu_available, monkeypatch, case, B=B)


@pytest.mark.gpu
def test_plans_of_the_ragged_handles(gpu_available, monkeypatch):
    """What the docstring says of the plans: the folds of the two-layer plan on the grid at every batch,
    none of them off it, the generic plan for three layers and above 512."""
    def names_of(case, B=64):
        _enter(monkeypatch, case)
        eng, *_ = D._pair(monkeypatch, case, B=B, seed=3)
        plan = eng.plan_info()
        eng.close()
        print(f"plan {case} B={B}: " + " ".join(f"{p['name']}[{p['kernel']}]" for p in plan))
        return [p["name"] for p in plan], [p["kernel"] for p in plan]

    for B in (1, 2, 15, 16, 17, 64):
        names, kern = names_of("grid2", B)
        assert "q.fwd01+actor.head" in names and "actor.head.bwd+actor.bwd1" in names and "actor.head" not in names, (B, names)
    names, _ = names_of("a32")             # 32 actions: the head keeps its launch, the actor's pair folds
    assert "q.head+critic.bwd1" in names and "actor.head" in names and "actor.fwd01" in names, names
    names, _ = names_of("off4")            # the actor on the grid (its head folds), the critics off it (no pair)
    assert "q.fwd0+actor.head" in names and "q.fwd1" in names and "actor.fwd01" in names, names
    assert "actor.head.bwd" in names and "pi.q.fwd01" not in names, names
    for case in ("odd2", "a31_odd", "tiny23"):
        names, kern = names_of(case, 17 if case == "odd2" else 64)
        assert "q.head+critic.bwd1" in names and "actor.head" in names and "actor.head.bwd" in names, (case, names)
        assert "k_fwd2" not in kern and not any("fwd01" in n or n.startswith("q.fwd0+") for n in names), (case, names)
    for case in ("odd_mid3", "odd_wide", "tiny1", "ln_wide_odd"):
        names, kern = names_of(case)
        assert not any("+" in n for n in names) and "k_fwd2" not in kern, (case, names)
        assert "actor.head" in names and "q.head" in names and "actor.head.bwd" in names, (case, names)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["odd_mid3", "tiny23"])
def test_trajectory_ragged(gpu_available, monkeypatch, case):
    """60 graph-replayed updates at B = 128 (the body of test_trajectory_any_depth): a wrong Adam v, weight
    write or Polyak in a ragged tail tile, which the first-moment check of one update cannot see."""
    _enter(monkeypatch, case)
    D.test_trajectory_any_depth(gpu_available, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["odd2", "eo_odd"])
def test_graph_equals_eager_ragged(gpu_available, monkeypatch, case):
    _enter(monkeypatch, case)
    D.test_graph_equals_eager_any_depth(gpu_available, monkeypatch, case)


DW_SHAPE = dict(hidden=(63, 64), critic_hidden=(66, 61))
# each Dense layer's dW problem: (the buffer holding the layer's input rows, the buffer holding its delta rows);
# the critics' head delta is the per-row loss gradient, B values of ws.gq read as one column (row stride 1: None)
DW_OPERANDS = {"q.l0": ("slot0.Xq", "ws.Dq1"), "q.l1": ("ws.Hq1", "ws.Dq2"), "q.l2": ("ws.Hq2", None),
               "actor.l0": ("slot0.Xa", "ws.Da1"), "actor.l1": ("ws.Ha1", "ws.Da2"), "actor.l2": ("ws.Ha2", "ws.Da3")}


def test_dw_tilings_ragged_strides_on_the_cpu():
    """No device: what test_dw_tilings_ragged's handle gives k_dwl's staging.  add_gemm stages an operand by
    16-B pieces when its row stride is a multiple of 4 and at least 4 (every buffer here begins 16-B aligned)
    and by dwords otherwise, so the (a4, b4) of a dW problem follows from the strides of its two buffers.  With
    A = 6 the actor head's delta rows (ws.Da3) are 6 wide, so this handle carries the three combinations with a
    dword-staged operand -- (1, 0), (0, 1), (0, 0) -- and (1, 1) stays with the 256-wide cases of
    test_gpu_dw.py.  A buffer whose stride changes shows here before the device test's coverage shrinks."""
    from sac_eo.engine import EngineConfig
    from test_ppo_config import _create, _layout
    lib, h, rc, msg = _create(EngineConfig(s_dim=17, a_dim=6, activation="relu", batch=128, buffer_capacity=5000,
                                           graph_steps=8, **DW_SHAPE).to_c())
    assert rc == 0, msg
    segs = _layout(lib, h)
    lib.sacx_destroy(h)
    v4 = lambda name: int(name is not None and segs[name][2] >= 4 and segs[name][2] % 4 == 0 and segs[name][0] % 16 == 0)
    combos = {layer: (v4(a), v4(b)) for layer, (a, b) in DW_OPERANDS.items()}
    print("k_dwl staging by layer:", combos, {n: segs[n][2] for ab in DW_OPERANDS.values() for n in ab if n})
    assert combos == {"q.l0": (1, 0), "q.l1": (0, 0), "q.l2": (0, 0), "actor.l0": (1, 0), "actor.l1": (0, 1),
                      "actor.l2": (1, 0)}, combos


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dwl32x16", "dwl32x32", "round"])
def test_dw_tilings_ragged(monkeypatch, variant):
    """test_dw_tilings_bit_identical at hidden (63, 64), critics (66, 61), B = 128, fp32: one handle with the
    three (a4, b4) combinations of k_dwl's staging that have a dword-staged operand -- layer 0 and the actor's
    head (1, 0), the actor's layer 1 (0, 1), the critics' layer 1 and head (0, 0); the strides behind that are
    held by test_dw_tilings_ragged_strides_on_the_cpu."""
    DW.test_dw_tilings_bit_identical(monkeypatch, variant, 128, False, False, **DW_SHAPE)


@pytest.mark.gpu
def test_packed_seeds_ragged(gpu_available):
    """Two seeds of (63, 65) against two single engines, bit for bit (the body of test_packed_seeds_wide)."""
    W.test_packed_seeds_wide(gpu_available, hidden=RAGGED["odd2"]["hidden"])


@pytest.mark.gpu
def test_bf16_update_ragged(gpu_available, monkeypatch):
    """bf16_parity's off4_bf16 (S=17, A=6, B=37, hidden (63, 65), elu) through the one-update body of
    test_gpu_bf16.py at bf16_parity.bars: an odd K leaves the last bf16 pair of a weight shadow row half
    filled.  Slabs: forward 2 (K = 17, 23) / 4 (K = 63: ragged); dX 5 (K = 65: odd, one element in the last
    slab); dW 3 (37 rows)."""
    BF._one_update("off4_bf16", monkeypatch, expect=("actor.head", "actor.head.bwd", "actor.bwd1", "critic.adam"),
                   absent=("q.fwd0+actor.head",))


FIT = {
    "odd": dict(model_hidden=(65, 127)),
    # a mixed launch: the model nets' problems load by float4, the reward nets' element-wise ...
    "srn_mixed_a": dict(model_hidden=(64, 64), wm=dict(separate_reward_nn=True, reward_hidden=(7, 9), reward_act="tanh")),
    # ... and the reverse
    "srn_mixed_b": dict(model_hidden=(63, 65), wm=dict(separate_reward_nn=True, reward_hidden=(64, 64), reward_act="tanh")),
    "gauss_odd": dict(model_hidden=(61,), wm=dict(gaussian_model=True)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FIT))
def test_model_fit_ragged(gpu_available, monkeypatch, case):
    """2 eager + 3 replayed fit steps, losses 1e-4, weights 5e-5, t_model, the plan check (the body of
    test_model_fit_any_depth)."""
    monkeypatch.setitem(D.FIT, case, dict(FIT[case], N=N))
    D.test_model_fit_any_depth(gpu_available, case)


@pytest.mark.gpu
@pytest.mark.parametrize("model_hidden", [(65, 127), (64, 100), (60, 36)], ids=lambda h: f"{h[0]}x{h[1]}")
def test_model_fit_folds_ragged(gpu_available, monkeypatch, model_hidden):
    """test_model_fit_folds_bit_identical at ragged model widths: every SACX_MFUSE / MTILE / MFWD2 / MT32 / MPRE
    variant bit-identical to the unfolded chain -- a fold either holds at the shape or declines.  The
    model.bwd2 fold (SACX_MFUSE=3) stores the generated layer-1 delta in 16-B pieces at row stride Hm1, one
    piece per lane of a 16-column slab: at Hm1 = 100 and 36 (multiples of 4, not of 16) the fold is taken and
    the last slab's pieces past the row must stay unwritten -- they would land on the next row, which another
    wave writes, and behind ws.Df2 -- and at 127 it declines."""
    E.test_model_fit_folds_bit_identical(gpu_available, monkeypatch, 17, 6, 64, 0.0, model_hidden=model_hidden)
    monkeypatch.setenv("SACX_MFUSE", "3")
    eng, *_ = make_pair(B=64, N=N, seed=33, use_expert=True, normalizers="random", model_hidden=model_hidden)
    names = [p["name"] for p in eng.model_plan_info()]
    eng.close()
    assert ("model.bwd2+bwd1+final" in names) == (model_hidden[1] % 4 == 0), names
    assert ("model.bwd2+final" in names) == (model_hidden[1] % 4 != 0), names


OBJ = dict(hidden=(63, 65), wm=dict(critic_hidden=(66, 61)), model_hidden=(65, 127))


@pytest.mark.gpu
def test_objects_ragged(gpu_available, monkeypatch):
    """evaluate, act on 3 and 40 rows, critic_forward / value, model_forward: 2e-5, the stream bit-exact (the
    body of test_objects_any_depth as test_objects_wide holds it)."""
    monkeypatch.setattr(W, "OBJ", OBJ)
    W.test_objects_wide(gpu_available)


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [False, True])
def test_rollout_ragged(gpu_available, monkeypatch, deterministic):
    monkeypatch.setattr(W, "OBJ", OBJ)
    W.test_rollout_wide(gpu_available, deterministic)


@pytest.mark.gpu
def test_expert_diag_ragged(gpu_available, monkeypatch):
    """The body of test_expert_diag_many_models with 2 world models (65, 127)."""
    monkeypatch.setattr(W, "OBJ", OBJ)
    W.test_expert_diag_wide(gpu_available, False)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,n", [((63, 65), 1), ((63, 65), 16), ((3, 1), 1)])
def test_act_rows_ragged(gpu_available, hidden, n):
    """k_act_rows (the prefetching path) on weight matrices whose rows are no whole number of 16-B pieces:
    the body of test_actor_act_rows_shapes."""
    E.test_actor_act_rows_shapes(gpu_available, 17, 6, "tanh", False, n, hidden=hidden)
