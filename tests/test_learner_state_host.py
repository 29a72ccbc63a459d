"""Full learner state, host side (learner_state.py, LearnerEngine.manifest, the agents' host_state): the container's bit-exact round
trip, what it refuses, its write order, the manifest comparison, and the per-rank files of data parallelism.  No GPU."""
import json
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from carla_driving_rl_agent_amd import learner_state as LS  # noqa: E402


def _awkward_arrays():
    """float32 bit patterns an arithmetic or text round trip would change: quiet and signalling NaNs with payloads, +-0, the
    smallest and largest denormals, +-inf, plus ordinary values."""
    bits = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0xff9abcde, 0x00000000, 0x80000000, 0x00000001, 0x807fffff,
                     0x007fffff, 0x7f800000, 0xff800000, 0x3f800000, 0xc2f6e979], dtype=np.uint32)
    rng = np.random.default_rng(3)
    return dict(params=np.concatenate([bits.view(np.float32), rng.standard_normal(1000).astype(np.float32)]),
                adam_m=bits[::-1].copy().view(np.float32), adam_v=np.full(7, 0.1, np.float32),
                m_cache=np.array([1.0, 0.4872, 3e-39], np.float32))


def _meta():
    rng = np.random.default_rng(11)
    rng.standard_normal(5)
    return dict(manifest=dict(optimizer='adam', polyak=1.0, tables={}), optimizer_steps=[3, 2, 5], action_index=17, sample_seed=24304,
                agent=dict(seed=7, rng=rng.bit_generator.state, numpy_random=LS.numpy_global_state(),
                           python_random=LS.python_random_state(random)))


def _files(path):
    return sorted(os.listdir(path))


def test_container_round_trip_is_bit_exact(tmp_path):
    arrays, meta = _awkward_arrays(), _meta()
    LS.save(str(tmp_path), arrays, meta)
    assert {'learner_state.index', 'learner_state.json'} <= set(_files(tmp_path))
    assert any(f.startswith('learner_state.data-') for f in _files(tmp_path))
    got, got_meta = LS.load(str(tmp_path))
    assert set(got) == set(arrays)
    for k, a in arrays.items():
        assert got[k].dtype == np.float32 and got[k].shape == a.shape
        assert got[k].tobytes() == a.tobytes(), k
    # a PCG64 state (two 128-bit integers) comes back equal, and a generator set to it continues the same stream
    assert got_meta['agent']['rng'] == meta['agent']['rng']
    assert got_meta['agent']['rng']['state']['state'] > 2 ** 64
    a, b = np.random.default_rng(0), np.random.default_rng(1)
    a.bit_generator.state = meta['agent']['rng']
    b.bit_generator.state = got_meta['agent']['rng']
    assert a.integers(2 ** 31, size=8).tolist() == b.integers(2 ** 31, size=8).tolist()
    for k in ('optimizer_steps', 'action_index', 'sample_seed', 'manifest'):
        assert got_meta[k] == meta[k]
    assert got_meta['version'] == LS.FORMAT_VERSION


def test_global_generator_states_round_trip_through_json():
    np.random.seed(5)
    random.seed(5)
    np.random.standard_normal(3)            # (leaves a cached gaussian behind: part of the state)
    random.gauss(0, 1)
    saved = json.loads(json.dumps(dict(n=LS.numpy_global_state(), p=LS.python_random_state(random))))
    want = (np.random.randint(0, 2 ** 31 - 1, size=4).tolist(), np.random.standard_normal(3).tolist(), [random.random() for _ in range(3)],
            random.gauss(0, 1))
    np.random.seed(99)
    random.seed(99)
    LS.set_numpy_global_state(saved['n'])
    LS.set_python_random_state(random, saved['p'])
    got = (np.random.randint(0, 2 ** 31 - 1, size=4).tolist(), np.random.standard_normal(3).tolist(), [random.random() for _ in range(3)],
           random.gauss(0, 1))
    assert got == want


def test_a_flipped_byte_in_the_data_shard_is_refused(tmp_path):
    LS.save(str(tmp_path), _awkward_arrays(), _meta())
    shard = tmp_path / 'learner_state.data-00001-of-00002'
    raw = bytearray(shard.read_bytes())
    raw[len(raw) // 2] ^= 0x10
    shard.write_bytes(bytes(raw))
    with pytest.raises(LS.LearnerStateError, match='crc32c'):
        LS.load(str(tmp_path))


def test_a_truncated_data_shard_is_refused(tmp_path):
    LS.save(str(tmp_path), _awkward_arrays(), _meta())
    shard = tmp_path / 'learner_state.data-00001-of-00002'
    shard.write_bytes(shard.read_bytes()[:-8])
    with pytest.raises(LS.LearnerStateError):
        LS.load(str(tmp_path))


def test_a_missing_json_is_an_incomplete_state(tmp_path):
    LS.save(str(tmp_path), _awkward_arrays(), _meta())
    os.unlink(tmp_path / 'learner_state.json')
    assert not LS.exists(str(tmp_path))
    with pytest.raises(LS.LearnerStateError, match='incomplete'):
        LS.load(str(tmp_path))


def test_an_unknown_version_is_refused(tmp_path):
    LS.save(str(tmp_path), _awkward_arrays(), _meta())
    path = tmp_path / 'learner_state.json'
    obj = json.loads(path.read_text())
    obj['version'] = LS.FORMAT_VERSION + 1
    path.write_text(json.dumps(obj))
    with pytest.raises(LS.LearnerStateError, match='version'):
        LS.load(str(tmp_path))
    LS.save_rank(str(tmp_path), 0, dict(agent={}))
    rank = tmp_path / 'learner_state.rank0.json'
    obj = json.loads(rank.read_text())
    obj['version'] = 'x'
    rank.write_text(json.dumps(obj))
    with pytest.raises(LS.LearnerStateError, match='version'):
        LS.load_rank(str(tmp_path), 0)


def _failing_json_replace(monkeypatch):
    real_replace = os.replace

    def failing_replace(src, dst):
        if str(dst).endswith('learner_state.json'):
            raise OSError(28, 'No space left on device')
        return real_replace(src, dst)
    monkeypatch.setattr(os, 'replace', failing_replace)


def test_failed_first_save_leaves_no_json_and_no_temporary_file(tmp_path, monkeypatch):
    _failing_json_replace(monkeypatch)
    with pytest.raises(OSError):
        LS.save(str(tmp_path), _awkward_arrays(), _meta())
    assert not [f for f in _files(tmp_path) if '.tmp' in f], _files(tmp_path)
    assert 'learner_state.json' not in _files(tmp_path)
    with pytest.raises(LS.LearnerStateError, match='incomplete'):
        LS.load(str(tmp_path))


def test_failed_save_leaves_the_previous_complete_state_readable(tmp_path, monkeypatch):
    first, meta = _awkward_arrays(), _meta()
    LS.save(str(tmp_path), first, meta)
    second = {k: np.arange(v.size, dtype=np.float32) for k, v in first.items()}
    with monkeypatch.context() as m:
        _failing_json_replace(m)
        with pytest.raises(OSError):
            LS.save(str(tmp_path), second, dict(meta, action_index=99))
    assert not [f for f in _files(tmp_path) if '.tmp' in f], _files(tmp_path)
    got, got_meta = LS.load(str(tmp_path))          # arrays AND json of the first save: never a mixture
    assert got_meta['action_index'] == meta['action_index']
    for k, a in first.items():
        assert got[k].tobytes() == a.tobytes(), k
    # the next save that succeeds replaces it, and the one after that goes back to the first file stem
    LS.save(str(tmp_path), second, dict(meta, action_index=99))
    got, got_meta = LS.load(str(tmp_path))
    assert got_meta['action_index'] == 99 and got['adam_v'].tobytes() == second['adam_v'].tobytes()
    LS.save(str(tmp_path), first, dict(meta, action_index=100))
    got, got_meta = LS.load(str(tmp_path))
    assert got_meta['action_index'] == 100 and got_meta['checkpoint'] == 'learner_state'
    assert got['adam_v'].tobytes() == first['adam_v'].tobytes()


def test_arrays_other_than_float32_are_refused(tmp_path):
    with pytest.raises(LS.LearnerStateError, match='float32'):
        LS.save(str(tmp_path), dict(params=np.zeros(3, np.float64)), {})
    assert _files(tmp_path) == []


# ------------------------------------------------------------------------------------------------ manifest
def _manifest(B, **kw):
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    return LearnerEngine(B, device=None, H=48, W=64, **kw).manifest()


def test_manifests_of_different_optimizers_are_incompatible():
    adam, sgd = _manifest(4, optimizer='adam'), _manifest(4, optimizer='sgd')
    diff = LS.manifest_difference(adam, sgd)
    assert diff is not None and 'optimizer' in diff and 'adam' in diff and 'sgd' in diff
    assert adam['tables'] == sgd['tables']          # (only the optimizer differs)


def test_manifests_do_not_depend_on_batch_size_or_mode_switches():
    a = _manifest(4, optimizer='adam')
    assert set(a['tables']) == {'trunk', 'policy', 'value'} and len(a['tables']['trunk']) > 300
    assert a['tables']['policy'][0][0] and isinstance(a['tables']['policy'][0][1], list)      # [name, shape, trainable, offset]
    for other in (_manifest(8, optimizer='adam'), _manifest(4, optimizer='adam', freeze_trunk=True),
                  _manifest(4, optimizer='adam', compute='bf16'), _manifest(4, optimizer='adam', train_stats=16)):
        assert LS.manifest_difference(a, other) is None
        assert LS.manifest_difference(json.loads(json.dumps(a)), other) is None      # (as it comes back from the JSON file)


def test_manifest_difference_names_the_first_table_entry_that_differs():
    a = _manifest(4)
    b = json.loads(json.dumps(a))
    b['tables']['value'][2][1] = [9, 9]
    diff = LS.manifest_difference(b, a)
    assert diff is not None and "'value'" in diff and 'entry 2' in diff and a['tables']['value'][2][0] in diff
    c = json.loads(json.dumps(a))
    c['tables']['trunk'].pop()
    assert 'entries' in LS.manifest_difference(c, a)


def test_host_only_engine_refuses_state_calls_clearly():
    from carla_driving_rl_agent_amd import _lib
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    eng = LearnerEngine(4, device=None, H=48, W=64)
    for call in (eng.export_state, lambda: eng.import_state({}), eng.get_optimizer_state):
        with pytest.raises(_lib.CdrlError, match='device=None'):
            call()


# ------------------------------------------------------------------------------------------------ per-rank files
def test_rank_file_names_and_absent_rank(tmp_path):
    base = str(tmp_path)
    assert os.path.basename(LS.rank_json_path(base, 3)) == 'learner_state.rank3.json'
    LS.save_rank(base, 0, dict(agent=dict(sample_offset=4)))
    LS.save_rank(base, 1, dict(agent=dict(sample_offset=6)))
    assert _files(tmp_path) == ['learner_state.rank0.json', 'learner_state.rank1.json']
    assert LS.load_rank(base, 1)['agent'] == dict(sample_offset=6) and LS.load_rank(base, 1)['rank'] == 1
    assert LS.load_rank(base, 2) is None            # the world grew: rank 2 wrote nothing


def _host_agent(monkeypatch, tmp_path, **kw):
    """A real CARLAgent whose learner engines are host-only (planned, never bound to a device)."""
    from carla_driving_rl_agent_amd.core import networks, CARLAgent, FakeCARLAEnvironment
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    monkeypatch.setattr(networks, 'LearnerEngine', lambda B, device=None, share_with=None, **cfg: LearnerEngine(B, device=None, share_with=share_with, **cfg))
    monkeypatch.setattr(networks, 'init_engine_parameters', lambda *a, **k: None)
    env = FakeCARLAEnvironment(image_shape=(48, 64, 3), time_horizon=2, num_waypoints=5, vehicle_features=4, num_actions=2,
                               image_range=(0.0, 1.0), seed=1)
    kw.setdefault('seed', 7)
    return CARLAgent(env, batch_size=4, log_mode=None, device='cpu', weights_dir=str(tmp_path), **kw)


def _draw(agent):
    """One draw from every generator an agent's host state covers, and the counters."""
    return (agent.seed, int(agent.rng.integers(2 ** 31)), float(agent._aug_rng.random()), int(np.random.randint(0, 2 ** 31 - 1)),
            random.random(), agent._sample_offset, agent._aug_calls, agent.network.action_index, agent.network.sample_seed)


def test_agent_host_state_restores_counters_and_every_generator(monkeypatch, tmp_path):
    agent = _host_agent(monkeypatch, tmp_path)
    assert agent.full_state is False
    agent._sample_offset, agent._aug_calls, agent.network.action_index = 5, 9, 12
    agent.rng.integers(10)
    agent._aug_rng.random(3)
    np.random.standard_normal(1)
    state = json.loads(json.dumps(agent.host_state()))
    want = _draw(agent)
    other = _host_agent(monkeypatch, tmp_path, seed=8)
    assert _draw(other) != want
    other.set_host_state(state)
    assert _draw(other) == want


def test_each_rank_restores_its_own_file_and_falls_back_without_one(monkeypatch, tmp_path, capsys):
    agent = _host_agent(monkeypatch, tmp_path)
    agent.data_parallel, agent.rank = True, 1
    assert agent.state_rank() == 1
    agent._sample_offset, agent._aug_calls = 6, 20
    steps = [2, 2, 2]
    LS.save_rank(agent.base_path, 1, dict(agent=agent.host_state(), optimizer_steps=steps))
    assert os.path.exists(os.path.join(agent.base_path, 'learner_state.rank1.json'))
    want = _draw(agent)
    meta = dict(optimizer_steps=steps, agent=dict(sample_offset=-1))          # (the writer's own host state is not a rank's)
    agent._sample_offset, agent._aug_calls = 0, 0
    agent.restore_host_state(meta)
    assert _draw(agent) == want
    # rank 2 has no file: it keeps what it has and says so in one line
    agent.rank = 2
    agent._sample_offset = 3
    capsys.readouterr()
    agent.restore_host_state(meta)
    out = capsys.readouterr().out
    assert agent._sample_offset == 3 and out.count('\n') == 1 and 'rank 2' in out and 'learner_state.rank2.json' in out
    # a rank file left behind by another save (other step counters) is not this state's
    agent.rank = 1
    agent.restore_host_state(dict(optimizer_steps=[4, 4, 4]))
    assert agent._sample_offset == 3 and 'rank 1' in capsys.readouterr().out
    # one process: the agent section of the state's own JSON
    agent.data_parallel = False
    state = agent.host_state()
    agent._sample_offset = 77
    agent.restore_host_state(dict(agent=json.loads(json.dumps(state))))
    assert agent._sample_offset == 3


def test_load_with_full_state_and_no_state_says_so_and_goes_on(monkeypatch, tmp_path, capsys):
    agent = _host_agent(monkeypatch, tmp_path, full_state=True)
    assert agent.full_state is True
    capsys.readouterr()
    assert agent.load_state(missing_ok=True) is False
    out = capsys.readouterr().out
    assert out.count('\n') == 1 and 'no learner state' in out
    with pytest.raises(LS.LearnerStateError):
        agent.load_state()
