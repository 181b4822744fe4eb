"""The step kernels' launch scalars (B, env_base, seed, K_done, auto_reset) arrive as kernel arguments, by
value, from the host copy in the context (csrc/futbol_kernels.hpp StepArgs) -- no longer through the
device params pointer.  Every case compares with the CPU oracle exactly, the way test_gpu_v1_parity.py
does: each of the five values in a setting where a wrong one shows (B = 1 and a last block of 63 shadow
lanes, a seed with a distinct high half, a large env base, episodes a few steps long with and without
auto-reset), two live contexts that differ in all of them on one stream and in one captured graph, and
the other compiled instances (runtime geometry, f64 outputs, rollout)."""
import numpy as np
import pytest
import torch

from helpers import O
from test_gpu_v1_parity import _compare_state

pytestmark = pytest.mark.gpu

SHORT = 0.45  # total_time / game_time of the short episodes


def _episode_steps(kind, limit):
    """the reference's episode length: envs_v1 adds 0.1 and then tests `current_time > total_time`; v0 tests
    `time >= game_time` first and then adds 0.1 (fp64 accumulation from 0, as the reference does)"""
    t, k = 0.0, 0
    while True:
        k += 1
        if kind == "v0" and t >= limit:
            return k
        t += 0.1
        if kind == "v1" and t > limit:
            return k


def _env(kind, B, seed, base=0, dtype=torch.float32, auto_reset=True, **kw):
    from gym_futbol_amd import FutbolVecEnv
    if kind == "v0":
        kw.setdefault("random_opp", False)
    return FutbolVecEnv(kind, B, seed=seed, env_id_base=base, dtype=dtype, auto_reset=auto_reset, **kw)


def _oracle(kind, B, seed, base=0, n=2, short=False, **kw):
    if kind == "v1":
        return O.V1Vec(B, N=n, seed=seed, env_id_base=base, portable=True, **(dict(total_time=SHORT) if short else {}),
                       **kw)
    return O.V0Vec(B, seed=seed, env_id_base=base, random_opp=False, portable=True,
                   **(dict(game_time=SHORT) if short else {}))


def _bits(x, dtype):
    """the oracle's f64 result as the bits of the kernel's output type"""
    if dtype == torch.float32:
        return np.asarray(x, np.float64).astype(np.float32).view(np.uint32)
    return np.asarray(x, np.float64).view(np.uint64)


def _same(gpu, cpu, dtype, what):
    g = gpu.cpu().numpy()
    assert np.array_equal(g.view(np.uint32 if dtype == torch.float32 else np.uint64), _bits(cpu, dtype)), what


def _acts(kind, a):
    a = a.cpu().numpy().astype(np.int32)
    return a if kind == "v1" else a.reshape(-1)


def _step_both(kind, venv, ora, t, dtype, tag, seed=1234):
    a = venv.random_actions(t, seed=seed)
    obs, rew, done, info = venv.step(a)
    o2, r2, d2, term2 = ora.step(_acts(kind, a))
    d1 = done.cpu().numpy()
    assert np.array_equal(d1, d2), "%s: done, step %d" % (tag, t)
    _same(rew, r2, dtype, "%s: reward, step %d" % (tag, t))
    _same(obs, o2, dtype, "%s: obs, step %d" % (tag, t))
    if d1.any():
        _same(info["terminal_observation"][done], term2[d2], dtype, "%s: terminal obs, step %d" % (tag, t))
    return d1


@pytest.mark.parametrize("kind", ["v1", "v0"])
@pytest.mark.parametrize("B", [1, 65])
def test_short_episodes_auto_reset(kind, B):
    """B = 1 (one live lane) and B = 65 (a last block of one live and 63 shadow lanes, clamped to env
    B - 1 with the by-value B), three episodes of 5 / 6 steps: K_done and auto_reset = 1 by value."""
    dt = torch.float32
    kw = {"total_time": SHORT, "number_of_player": 2} if kind == "v1" else {"game_time": SHORT}
    venv, ora = _env(kind, B, 31, **kw), _oracle(kind, B, 31, short=True)
    _same(venv.reset(), ora.reset(), dt, "reset")
    L = venv.episode_steps
    assert L == _episode_steps(kind, SHORT) == (5 if kind == "v1" else 6)
    ends = []
    for t in range(3 * L):
        d = _step_both(kind, venv, ora, t, dt, "%s B=%d" % (kind, B))
        assert d.all() == d.any()
        if d.all():
            ends.append(t)
    assert ends == [L - 1, 2 * L - 1, 3 * L - 1]
    if kind == "v1":
        _compare_state(venv, ora, 2, B, "end")
    assert np.array_equal(venv.get_state()["stat_cnt"], np.full(B, 3, np.uint32))
    venv.close()


@pytest.mark.parametrize("kind", ["v1", "v0"])
@pytest.mark.parametrize("B", [1, 65])
def test_short_episodes_without_auto_reset(kind, B):
    """auto_reset = 0 by value: `done` is set from the episode's last step on and nothing resets.  The
    reference is the oracle of the same envs with the default, long episode (neither kind's dynamics or
    reward depend on the time limit, only `done` does): every observation and reward, through the end and
    three steps past it, is that oracle's bit for bit -- at the last step the short-episode oracle's
    terminal_observation too -- the step counter goes on, and the RNG event counter moves by one per step
    (a reset takes one more)."""
    dt = torch.float32
    kw = {"total_time": SHORT, "number_of_player": 2} if kind == "v1" else {"game_time": SHORT}
    venv = _env(kind, B, 32, dtype=dt, auto_reset=False, **kw)
    short, long_ = _oracle(kind, B, 32, short=True), _oracle(kind, B, 32)
    o0 = long_.reset()
    short.reset()
    _same(venv.reset(), o0, dt, "reset")
    L = venv.episode_steps
    assert L == _episode_steps(kind, SHORT)
    ev0 = venv.get_state()["meta"].astype(np.uint64) >> np.uint64(32)
    for t in range(L + 3):
        a = venv.random_actions(t)
        obs, rew, done, _ = venv.step(a)
        o2, r2, d2, _ = long_.step(_acts(kind, a))
        assert not d2.any()
        assert bool(done.all()) == bool(done.any()) == (t >= L - 1), "done from the last step on, step %d" % t
        _same(rew, r2, dt, "reward, step %d" % t)
        _same(obs, o2, dt, "obs, step %d" % t)
        if t < L:
            _, r3, d3, term3 = short.step(_acts(kind, a))
            assert bool(d3.all()) == (t == L - 1)
            _same(rew, r3, dt, "reward (short-episode oracle), step %d" % t)
            if t == L - 1:
                _same(obs, term3, dt, "the terminal observation")
        meta = venv.get_state()["meta"].astype(np.uint64)
        assert np.array_equal((meta >> np.uint64(18)) & np.uint64(0x3FFF), np.full(B, t + 1, np.uint64)), "steps go on"
        assert np.array_equal(meta >> np.uint64(32), ev0 + np.uint64(t + 1)), "one RNG event per step: no reset"
    if kind == "v1":
        _compare_state(venv, long_, 2, B, "three steps past the end")
    venv.close()


@pytest.mark.parametrize("kind", ["v1", "v0"])
def test_seed_high_half_and_env_base(kind):
    """seed 0x9E3779B97F4A7C15 (the high half differs from the low one) with env_id_base 3 * 2^20 + 7: the
    64-bit seed and the base by value.  Against the oracle, and env i of a context based at b equals env
    i - k of a context based at b + k."""
    seed, base, B, k = 0x9E3779B97F4A7C15, 3 * 2**20 + 7, 64, 5
    dt = torch.float64
    kw = {"number_of_player": 2} if kind == "v1" else {}
    a_env, b_env = _env(kind, B, seed, base, dt, **kw), _env(kind, B, seed, base + k, dt, **kw)
    ora = _oracle(kind, B, seed, base)
    o_a, o_b = a_env.reset(), b_env.reset()
    _same(o_a, ora.reset(), dt, "reset")
    assert torch.equal(o_a[k:], o_b[:B - k])
    for t in range(20):
        act = a_env.random_actions(t)
        oa, ra, da, _ = a_env.step(act)
        o2, r2, d2, _ = ora.step(_acts(kind, act))
        _same(oa, o2, dt, "obs, step %d" % t)
        _same(ra, r2, dt, "reward, step %d" % t)
        act_b = torch.zeros_like(act)
        act_b[:B - k] = act[k:]
        ob, rb, db, _ = b_env.step(act_b)
        assert torch.equal(oa[k:], ob[:B - k]) and torch.equal(ra[k:], rb[:B - k]) and torch.equal(da[k:], db[:B - k]), t
    if kind == "v1":
        _compare_state(a_env, ora, 2, B, "end")
    # the low half alone, or another base, is another trajectory (the comparison above is not vacuous)
    other = _oracle(kind, B, seed & 0xFFFFFFFF, base)
    other.reset()
    ora2 = _oracle(kind, B, seed, base)
    ora2.reset()
    differs = False
    for t in range(20):
        act = _acts(kind, a_env.random_actions(t))
        differs = differs or not np.array_equal(other.step(act)[0], ora2.step(act)[0])
    assert differs
    a_env.close()
    b_env.close()


def test_two_live_contexts_stepped_and_captured_together():
    """Two contexts that differ in N (2 / 3), B (65 / 128), seed, base and auto_reset, stepped alternately
    on one stream, then captured together in one graph and replayed 3 times: each launch carries its own
    context's values, and each context matches its own oracle."""
    dt = torch.float32
    e2 = _env("v1", 65, 0x1234567811, 11, dt, True, number_of_player=2, total_time=SHORT)
    e3 = _env("v1", 128, 77, 4096, dt, False, number_of_player=3, total_time=0.75)
    o2 = O.V1Vec(65, N=2, seed=0x1234567811, env_id_base=11, total_time=SHORT, portable=True)
    o3 = O.V1Vec(128, N=3, seed=77, env_id_base=4096, total_time=0.75, portable=True)
    _same(e2.reset(), o2.reset(), dt, "reset 2v2")
    _same(e3.reset(), o3.reset(), dt, "reset 3v3")
    assert (e2.episode_steps, e3.episode_steps) == (5, 8)
    for t in range(4):  # alternately, eager
        _step_both("v1", e2, o2, t, dt, "2v2")
        d3 = _step_both("v1", e3, o3, t, dt, "3v3")
        assert not d3.any()
    # one graph of both contexts' steps, on static action buffers
    a2, a3 = torch.zeros_like(e2._act), torch.zeros_like(e3._act)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            e2.step_raw(a2)
            e3.step_raw(a3)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    # (capture records the launches without running them: the envs are still at step 4)
    for t in range(4, 7):
        a2.copy_(e2.random_actions(t, seed=9))
        a3.copy_(e3.random_actions(t, seed=9))
        g.replay()
        torch.cuda.synchronize()
        for e, o, a, tag in ((e2, o2, a2, "2v2"), (e3, o3, a3, "3v3")):
            ob, r, d, term = o.step(a.cpu().numpy().astype(np.int32))
            assert np.array_equal(e._done.cpu().numpy().astype(bool), d), (tag, t)
            _same(e._rew, r, dt, "%s replay: reward, step %d" % (tag, t))
            # 3v3 runs without auto-reset: no episode of its 8 steps ends here; 2v2 resets at step 4
            _same(e._obs, ob, dt, "%s replay: obs, step %d" % (tag, t))
            if d.any():
                _same(e._term[e._done.bool()], term[d], dt, "%s replay: terminal obs" % tag)
        assert bool(e2._done.all()) == (t == 4)
    _compare_state(e2, o2, 2, 65, "2v2 end")
    _compare_state(e3, o3, 3, 128, "3v3 end")
    e2.close()
    e3.close()


def test_runtime_geometry_f64_and_rollout():
    """The other compiled step instances at B = 65: runtime geometry (width 90, height 60) with f64
    outputs against the oracle, and rollout(nsteps = 3) equal to 3 steps (both geometries, v0 too)."""
    B, dt = 65, torch.float64
    kw = dict(number_of_player=2, width=90, height=60)
    venv = _env("v1", B, 5, 3, dt, **kw)
    ora = O.V1Vec(B, N=2, seed=5, env_id_base=3, width=90.0, height=60.0, portable=True)
    _same(venv.reset(), ora.reset(), dt, "reset 90x60")
    for t in range(6):
        _step_both("v1", venv, ora, t, dt, "90x60")
    _compare_state(venv, ora, 2, B, "90x60")
    venv.close()
    for kind, kw in (("v1", kw), ("v1", dict(number_of_player=2)), ("v0", {})):
        a, b = _env(kind, B, 6, 3, dt, **kw), _env(kind, B, 6, 3, dt, **kw)
        a.reset()
        b.reset()
        acts = a.random_actions_steps(3, 0, seed=8)
        obs, rew, done, _ = b.rollout(acts)
        for k in range(3):
            o, r, d, _ = a.step(acts[k])
            assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d.to(torch.uint8), done[k]), (kind, k)
        sa, sb = a.get_state(), b.get_state()
        assert all(np.array_equal(sa[f], sb[f]) for f in sa), kind
        a.close()
        b.close()
