"""Device-resident trace sets at the agent level (rl/trace_set.py): twin agents as in tests/test_gpu_imitate.py --
48x64, time_horizon 4, two actions, a per-step trace of 19 rows and a stacked one of 24, minibatches of 8.  One agent learns from the
files, its twin from the set: weights, optimizer slots, old policy, generator state and logged losses must be equal BIT FOR BIT.
`camera` is the same directory with images of the form q / 255, so the byte-coded image path runs through an agent."""
import os

import numpy as np
import pytest
import torch

from carla_driving_rl_agent_amd import traces
from carla_driving_rl_agent_amd.rl.trace_set import TraceSet, TraceSpec
from tests import test_gpu_imitate as base

pytestmark = pytest.mark.gpu
DEV, T, A, BATCH, KEYS, ARENAS = base.DEV, base.T, base.A, base.BATCH, base.KEYS, base.ARENAS
_agent = base._agent


@pytest.fixture(scope='module')
def dirs(tmp_path_factory):
    both, camera = str(tmp_path_factory.mktemp('both')), str(tmp_path_factory.mktemp('camera'))
    for path in (both, camera):
        base._record(path, 1, 19, seed=11, time_axis=False)
        base._record(path, 2, 24, seed=12, time_axis=True)
    for name in traces.trace_files(camera):
        with np.load(os.path.join(camera, name)) as f:
            trace = {k: f[k] for k in f.keys()}
        q = np.clip(np.floor((trace['state_image'] + 1.0) * 127.5), 0, 255).astype(np.float32)         # the environment draws in [-1, 1]
        trace['state_image'] = q / np.float32(255.0)
        np.savez_compressed(os.path.join(camera, name), **trace)
    return both, camera


def _twins(tmp_path, **kw):
    agent, twin = _agent(tmp_path, **kw), _agent(tmp_path, name='twin', **kw)
    logs = []
    for who in (agent, twin):
        rows = []
        who.log = lambda _rows=rows, **entry: _rows.append(sorted(entry.items()))
        logs.append(rows)
    return agent, twin, logs


def _same(agent, twin, logs):
    torch.cuda.synchronize()
    a, b = agent.network.engine, twin.network.engine
    for name in ARENAS:         # params holds policy, value, trunk, old_policy and the moving statistics
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert agent.rng.bit_generator.state == twin.rng.bit_generator.state
    assert logs[0] == logs[1] and len(logs[0]) > 0


def _weights(trace):
    n = trace['action'].shape[0]
    return np.linspace(0.5, 1.5, n, dtype=np.float32)


@pytest.mark.parametrize('which,value_weight,weights', [(0, 0.0, None), (0, 0.5, None), (0, 0.5, _weights), (1, 0.5, None)],
                         ids=['actions', 'value', 'weights', 'camera-bytes'])
def test_imitate_from_a_set_is_imitate_from_files(tmp_path, dirs, which, value_weight, weights):
    agent, twin, logs = _twins(tmp_path)
    fresh = agent.network.engine.params.clone()
    agent.imitate(epochs=2, traces_dir=dirs[which], value_weight=value_weight, weights=weights, close=False)
    ts = twin.load_trace_set(dirs[which], weights=weights)
    assert ts.codes['state_image'] == ('u8' if which else 'f32') and ts.codes['state_road'] == 'u8'
    assert (ts.rows, ts.traces, ts.has_weight) == (43, 2, weights is not None)
    twin.imitate(epochs=2, trace_set=ts, value_weight=value_weight, close=False)
    _same(agent, twin, logs)
    assert len(logs[0]) == 2 * 6 and not torch.equal(agent.network.engine.params, fresh)
    assert ('imitation_loss_value' in dict(logs[0][0])) == (value_weight > 0.0)


def test_max_traces_and_another_gamma(tmp_path, dirs):
    """max_traces cuts the epoch's drawn order as the file path cuts it; an agent with another discount gets the returns of ITS gamma
    from the stored rewards."""
    agent, twin, logs = _twins(tmp_path, gamma=0.9)
    donor = _agent(tmp_path, name='donor')                      # gamma 0.99: the set's own returns are not the twins'
    ts = donor.load_trace_set(dirs[0])
    assert ts.gamma == donor.gamma != twin.gamma
    agent.imitate(epochs=2, traces_dir=dirs[0], value_weight=0.5, max_traces=1, close=False)
    twin.imitate(epochs=2, trace_set=ts, value_weight=0.5, max_traces=1, close=False)
    _same(agent, twin, logs)
    assert len(logs[0]) == 2 * 3


def test_learn_representation_from_a_set(tmp_path, dirs):
    agent, twin, logs = _twins(tmp_path)
    agent.learn_representation(epochs=2, traces_dir=dirs[0], intensity=0.5)
    twin.learn_representation(epochs=2, traces_dir=twin.load_trace_set(dirs[0]), intensity=0.5)
    _same(agent, twin, logs)


def test_score_traces_from_a_set(tmp_path, dirs):
    agent = _agent(tmp_path)
    agent.learn(episodes=1, timesteps=12, close=False)          # moving statistics off their initial values
    ts = agent.load_trace_set(dirs[0])
    for kw in (dict(), dict(per_trace=True), dict(chunk=5, value=False), dict(max_traces=1, aux=False)):
        want, got = agent.score_traces(dirs[0], **kw), agent.score_traces(ts, **kw)
        assert np.array_equal(want['block'], got['block']) and want['rows'] == got['rows']
        if kw.get('per_trace'):
            assert len(got['traces']) == 2
            for w, g in zip(want['traces'], got['traces']):
                assert np.array_equal(w['block'], g['block'])


def test_validation_on_a_held_out_set(tmp_path, dirs):
    agent, twin, logs = _twins(tmp_path)
    agent.imitate(epochs=2, traces_dir=dirs[0], validation_dir=dirs[1], close=False)
    twin.imitate(epochs=2, trace_set=twin.load_trace_set(dirs[0]), validation_set=twin.load_trace_set(dirs[1]), close=False)
    _same(agent, twin, logs)
    assert sum('validation_log_prob' in dict(e) for e in logs[0]) == 2


def test_mixed_minibatches_are_the_written_out_loop(tmp_path, dirs):
    value_weight = 0.5
    agent, twin, _ = _twins(tmp_path)
    ts = agent.load_trace_set(dirs[0])
    agent.imitate(trace_set=ts, mix_traces=True, value_weight=value_weight, close=False)
    # the loop: the file path's tensors one trace behind the other, one generator draw, a true permutation, rows by torch indexing
    net = twin.network
    net.set_hparams(**twin.hyper_parameters())
    parts = [twin._trace_tensors(trace, None, True, value_weight) for trace in traces.load_traces(dirs[0])]
    cat = lambda pick: torch.cat([pick(p) for p in parts], dim=0)
    whole = dict(states={k: cat(lambda p, k=k: p['states'][k]) for k in KEYS},
                 **{c: cat(lambda p, c=c: p[c]) for c in ('u', 'speed', 'similarity', 'returns')})
    order = np.random.default_rng(int(twin.rng.integers(2 ** 31))).permutation(43)
    sizes, both = [], 0
    for lo in range(0, 43, BATCH):
        rows = order[lo:lo + BATCH]
        both += rows.min() < 19 <= rows.max()
        index = torch.as_tensor(rows, device=DEV).long()
        b = dict(states={k: v[index].contiguous() for k, v in whole['states'].items()},
                 **{c: whole[c][index].contiguous() for c in ('u', 'speed', 'similarity', 'returns')})
        eng = net.engine_for(len(rows))
        eng.clone_step(eng.stage(b, 'clone'), 1.0, value_weight, 1.0)
        sizes.append(len(rows))
    net.update_old_policy()
    assert sizes == [8, 8, 8, 8, 8, 3] and both >= 1            # a ragged tail; minibatches that hold rows of both traces
    torch.cuda.synchronize()
    a, b = agent.network.engine, twin.network.engine
    for name in ARENAS:
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert agent.rng.bit_generator.state == twin.rng.bit_generator.state
    # the representation stage draws its batch_size / 2 rows the same way: it runs, learns and leaves the heads alone
    heads = a.params[base._slice(a, 'policy')].clone()
    before = a.params.clone()
    agent.learn_representation(traces_dir=ts, shuffle_data='set', intensity=0.5)
    assert torch.isfinite(a.params).all() and not torch.equal(a.params, before)
    assert torch.equal(a.params[base._slice(a, 'policy')], heads)


def test_files_are_opened_once_at_load(tmp_path, dirs, monkeypatch):
    agent, twin, logs = _twins(tmp_path)
    opened, load = [], np.load

    def counting(file, *args, **kw):
        opened.append(os.path.basename(str(file)))
        return load(file, *args, **kw)

    monkeypatch.setattr(np, 'load', counting)
    names = traces.trace_files(dirs[0])
    agent.imitate(epochs=3, traces_dir=dirs[0], close=False)
    assert sorted(opened) == sorted(names * 3)                  # the file path: every file, every epoch
    del opened[:]
    ts = twin.load_trace_set(dirs[0])
    assert opened == names                                      # each once, in sorted order
    twin.imitate(epochs=3, trace_set=ts, close=False)
    twin.score_traces(ts)
    assert opened == names                                      # and never again
    _same(agent, twin, logs)


def test_loading_a_set_touches_nothing_of_the_agent(tmp_path, dirs):
    agent = _agent(tmp_path)
    agent.learn(episodes=1, timesteps=12, close=False)
    eng = agent.network.engine
    torch.cuda.synchronize()
    before = {name: getattr(eng, name).clone() for name in ARENAS}
    state = (agent._sample_offset, agent.network.action_index, agent.rng.bit_generator.state)
    ts = agent.load_trace_set(dirs[0])
    ts.trace_tensors(1)
    ts.batch(ts.upload_index(np.arange(43)[::-1]), 3, 17)
    torch.cuda.synchronize()
    for name in ARENAS:
        assert torch.equal(before[name], getattr(eng, name)), name
    assert state == (agent._sample_offset, agent.network.action_index, agent.rng.bit_generator.state)


def test_batches_are_the_file_tensors(tmp_path, dirs):
    """trace_tensors and batch against PPOAgent._trace_tensors per file; storage='f16' is float32(float16(x)) of the image alone."""
    agent = _agent(tmp_path)
    bits = lambda t: t.contiguous().view(torch.int32)
    loaded = list(traces.load_traces(dirs[0]))
    files = [agent._trace_tensors(trace, _weights, True, 1.0) for trace in loaded]
    ts = agent.load_trace_set(dirs[0], weights=_weights)
    for i, want in enumerate(files):
        got = ts.trace_tensors(i)
        assert sorted(got) == sorted(want) == ['returns', 'similarity', 'speed', 'states', 'u', 'weight']
        for k in KEYS:
            assert got['states'][k].shape == want['states'][k].shape and torch.equal(bits(got['states'][k]), bits(want['states'][k])), k
        for c in ('u', 'weight', 'speed', 'similarity', 'returns'):
            assert got[c].shape == want[c].shape and got[c].is_contiguous() and torch.equal(bits(got[c]), bits(want[c])), c
        assert sorted(ts.trace_tensors(i, ('u',))) == ['states', 'u'] and list(ts.trace_tensors(i, ())) == ['states']
    order = np.random.default_rng(1).integers(0, 43, 60)                          # duplicates, both traces
    got = ts.batch(ts.upload_index(order), 7, 50)
    pick = torch.as_tensor(order[7:57], device=DEV).long()
    for k in KEYS:
        assert torch.equal(bits(got['states'][k]), bits(torch.cat([f['states'][k] for f in files])[pick])), k
    for c in ('u', 'weight', 'speed', 'similarity', 'returns'):
        assert torch.equal(bits(got[c]), bits(torch.cat([f[c] for f in files])[pick])), c
    half = agent.load_trace_set(dirs[0], storage='f16')
    assert half.codes['state_image'] == 'f16' and {k: half.codes[k] for k in KEYS[1:]} == {k: ts.codes[k] for k in KEYS[1:]}
    assert half.nbytes['state_image']['bytes'] * 2 == ts.nbytes['state_image']['bytes']
    for i, (trace, want) in enumerate(zip(loaded, files)):
        got = half.trace_tensors(i)['states']
        n = trace['action'].shape[0]
        image = trace['state_image'].astype(np.float16).astype(np.float32)
        if image.ndim == 4:
            image = image[traces.window_index(n, T).reshape(n, T)]
        assert np.array_equal(got['state_image'].cpu().numpy().view(np.int32), image.view(np.int32))
        for k in KEYS[1:]:
            assert torch.equal(bits(got[k]), bits(want['states'][k])), k


def _three_actions(tmp_path) -> str:
    path = str(tmp_path / 'wide')
    base._record(path, 1, 8, seed=5, time_axis=True, actions=np.zeros((8, 3), np.float32))
    return path


def test_what_a_set_refuses(tmp_path, dirs):
    agent = _agent(tmp_path)
    ts = agent.load_trace_set(dirs[0])
    before = agent.network.engine.params.clone()
    with pytest.raises(ValueError, match='not both'):
        agent.imitate(traces_dir=dirs[0], trace_set=ts, close=False)
    with pytest.raises(ValueError, match='needs trace_set'):
        agent.imitate(traces_dir=dirs[0], mix_traces=True, close=False)
    with pytest.raises(ValueError, match='needs a trace set'):
        agent.learn_representation(traces_dir=dirs[0], shuffle_data='set')
    with pytest.raises(ValueError, match="True, False or 'set'"):
        agent.learn_representation(traces_dir=ts, shuffle_data='rows')
    with pytest.raises(ValueError, match='per-trajectory'):
        agent.learn_representation(traces_dir=ts, shuffle_data='set', max_traces=1)
    with pytest.raises(ValueError, match='when it is loaded'):
        agent.imitate(trace_set=ts, weights=_weights, close=False)
    with pytest.raises(ValueError, match='per-trajectory'):
        agent.imitate(trace_set=ts, mix_traces=True, max_traces=1, close=False)
    with pytest.raises(ValueError, match='validation_dir or validation_set'):
        agent.imitate(trace_set=ts, validation_dir=dirs[1], validation_set=ts, close=False)
    with pytest.raises(ValueError, match=r'outside 0\.\.42'):
        ts.upload_index([0, 43])
    with pytest.raises(ValueError, match='rows \\['):
        ts.batch(ts.upload_index([0, 1, 2]), 2, 2)
    with pytest.raises(ValueError, match='int32'):
        ts.batch(torch.zeros(4, dtype=torch.int64, device=DEV), 0, 2)
    bare = str(tmp_path / 'bare')
    base._record(bare, 1, 8, seed=5, time_axis=True, info=False)
    plain = agent.load_trace_set(bare)
    assert not plain.has_info and plain.has_value
    with pytest.raises(ValueError, match='value_weight=0 and aux_weight=0'):
        agent.imitate(trace_set=plain, close=False)
    narrow = TraceSet.from_dir(TraceSpec({k: agent.state_spec[k] for k in KEYS}, T, A + 1, -1.0, 1.0, device=DEV),
                               _three_actions(tmp_path), upload=False)
    with pytest.raises(ValueError, match='load it with this agent'):
        agent.imitate(trace_set=narrow, close=False)
    agent.data_parallel = True
    try:
        with pytest.raises(RuntimeError, match='one GPU'):
            agent.imitate(trace_set=ts, close=False)
        with pytest.raises(RuntimeError, match='one GPU'):
            agent.score_traces(ts)
    finally:
        agent.data_parallel = False
    torch.cuda.synchronize()
    assert torch.equal(before, agent.network.engine.params)
    agent.imitate(trace_set=plain, aux_weight=0.0, value_weight=0.0, close=False)          # the actions alone
    assert torch.isfinite(agent.network.engine.params).all() and not torch.equal(before, agent.network.engine.params)


def test_bench_tool_runs_and_reports_its_keys(tmp_path):
    """tools/bench_traceset.py at a tiny size: it runs, and its JSON has the keys the documents quote.  No figure is judged."""
    import json
    import subprocess
    import sys
    out = tmp_path / 'bench.json'
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, 'tools', 'bench_traceset.py'), '--rows', '64', '--height', '48', '--width', '64',
                    '--epochs', '1', '--batch', '8', '--blocks', '1', '--reps', '2', '--out', str(out)], check=True, timeout=300,
                   stdout=subprocess.DEVNULL)
    got = json.loads(out.read_text())
    assert {'imitate', 'minibatch', 'storage', 'not_measured', 'device'} <= set(got)
    assert {'imitate_from_files_ms', 'imitate_from_trace_set_ms', 'trace_set_build_ms', 'same_bits', 'rows'} <= set(got['imitate'])
    assert {'launch_ms', 'gather_rows_ms', 'bytes_written', 'bytes_read_launch', 'launch_gbytes_per_s', 'same_bits'} <= set(got['minibatch'])
    assert {'nbytes', 'windowed_float32_bytes', 'ratio'} <= set(got['storage']) and got['storage']['nbytes']['state_image']['code'] == 'u8'
    assert got['imitate']['same_bits'] and got['minibatch']['same_bits']
