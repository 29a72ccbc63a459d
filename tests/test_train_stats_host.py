"""Update diagnostics ("train stats") on the host: the row layout the planner reports against the parameter table, the decoding of
a ring block, and the mapping of rows to the reference's log keys (tests/golden/ref_update_log_keys.json: the keyword names of every
self.log(...) call on the reference's update path, extracted by tests/golden/make_update_log_keys.py).  No GPU."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ref_update_log_keys.json')


def _engine(B=4, **kw):
    from carla_driving_rl_agent_amd.engine import LearnerEngine
    return LearnerEngine(B, device=None, H=48, W=64, **kw)


def _names(eng):
    return {m: [e['name'] for e in eng.tables[m].entries if e['trainable']] for m in ('policy', 'value', 'trunk')}


def _synthetic_rows(names, frozen=False):
    pn = {n: 0.5 + i for i, n in enumerate(names['policy'])}
    vn = {n: 0.25 + i for i, n in enumerate(names['value'])}
    tn = {} if frozen else {n: 1.0 + 0.001 * i for i, n in enumerate(names['trunk'])}
    policy = dict(kind='policy', t_head=3, t_dynamics=6, lr=1e-3, lr_dynamics=2e-3, clip_ratio=0.2, entropy_coef=0.3, speed=1.1,
                  similarity=-0.2, norms=pn, trunk_norms=dict(tn),
                  metrics=dict(loss=0.9, policy_loss=0.4, entropy=-1.5, speed_loss=0.05, similarity_loss=0.07, ratio=1.01, log_prob=0.8))
    value = dict(kind='value', t_head=3, t_dynamics=7, lr=3e-4, lr_dynamics=2e-3, clip_ratio=0.2, entropy_coef=0.3, speed=0.9,
                 similarity=0.1, norms=vn, trunk_norms=dict(tn),
                 metrics=dict(loss=0.6, value_loss=2.0, speed_loss=0.3, similarity_loss=0.1))
    return [policy, value]


def test_rows_map_to_exactly_the_reference_keys():
    from carla_driving_rl_agent_amd import train_stats as ts
    golden = json.load(open(GOLDEN))
    assert len(golden) == 26 and len(set(golden)) == 26
    names = _names(_engine())
    rows = _synthetic_rows(names)
    entries = ts.log_entries(rows)
    actions = np.array([[0.0, 1.0], [0.5, 0.25], [1.0, 0.75]], np.float32)
    act = ts.action_entries(actions)
    produced = set(act)
    for kw in entries:
        produced |= set(kw)
    assert produced == set(golden), produced ^ set(golden)
    pol, val = entries
    # each gradients_norm_* value is a list with one norm per tensor, in table order
    assert pol['gradients_norm_policy'] == [0.5 + i for i in range(len(names['policy']))]
    assert val['gradients_norm_value'] == [0.25 + i for i in range(len(names['value']))]
    assert len(pol['gradients_norm_dynamics']) == len(val['gradients_norm_dynamics_v']) == len(names['trunk']) == 264
    assert 'gradients_norm_value' not in pol and 'gradients_norm_policy' not in val
    # spot values against the reference's expressions
    assert pol['loss_entropy'] == float(np.float32(0.3) * np.float32(-1.5))          # entropy_strength() * entropy
    assert pol['loss_total'] == 0.9 and pol['loss_policy'] == 0.4 and pol['lr_policy'] == 1e-3
    assert pol['loss_speed_policy'] == 0.05 and pol['loss_similarity_policy'] == 0.07   # (the engine's terms carry the 0.5)
    assert pol['ratio_clip'] == 0.2 and pol['entropy_coeff'] == 0.3 and pol['speed_pi'] == 1.1 and pol['similarity_pi'] == -0.2
    assert val['loss_value'] == 0.6 and val['loss_v'] == 2.0 and val['loss_speed_value'] == 0.3
    assert val['loss_similarity_value'] == 0.1 and val['speed_v'] == 0.9 and val['similarity_v'] == 0.1 and val['lr_value'] == 3e-4
    # (actions - 1) * 2 + 1
    assert np.array_equal(act['action_throttle_or_brake'], np.array([-1.0, 0.0, 1.0], np.float32))
    assert np.array_equal(act['action_steer'], np.array([1.0, -0.5, 0.5], np.float32))
    assert ts.action_entries(actions[:, :1]) is None
    # what update() logs itself is left out on request, nothing else
    skipped = ts.log_entries(rows, skip=ts.LOGGED_BY_UPDATE)
    assert (set(skipped[0]) | set(skipped[1])) == set(golden) - set(ts.LOGGED_BY_UPDATE) - set(act)


def test_frozen_rows_carry_no_dynamics_keys():
    from carla_driving_rl_agent_amd import train_stats as ts
    names = _names(_engine())
    pol, val = ts.log_entries(_synthetic_rows(names, frozen=True))
    assert 'gradients_norm_dynamics' not in pol and 'gradients_norm_dynamics_v' not in val
    assert len(pol['gradients_norm_policy']) == len(names['policy'])


@pytest.mark.parametrize('frozen', [False, True])
def test_layout_against_the_parameter_table(frozen):
    off = _engine(freeze_trunk=frozen)
    assert off.train_stats_layout['rows'] == 0 and off.train_stats_layout['width'] == 0 and off.train_stats() is None
    eng = _engine(train_stats=5, freeze_trunk=frozen)
    L, names = eng.train_stats_layout, _names(eng)
    assert L['rows'] == 5 and L['header'] >= 2
    assert L['n_policy'] == len(names['policy']) and L['n_value'] == len(names['value'])
    assert L['n_trunk'] == (0 if frozen else len(names['trunk']))
    # fields do not overlap and fit the row
    spans = [(L[k], 1) for k in ('kind', 't_head', 't_dynamics', 'lr', 'lr_dynamics', 'clip_ratio', 'entropy_coef', 'speed', 'similarity')]
    spans += [(L['metrics'], 16), (L['norms'], max(L['n_policy'], L['n_value'])), (L['trunk_norms'], L['n_trunk'])]
    used = np.zeros(L['width'], int)
    for o, n in spans:
        assert 0 <= o and o + n <= L['width'], (o, n, L['width'])
        used[o:o + n] += 1
    assert used.max() == 1
    # the ring costs workspace only when it is on; tables and arenas are those of the plain engine
    assert eng.workspace_bytes > off.workspace_bytes
    assert eng.workspace_bytes - off.workspace_bytes < (1 << 20)
    for m in ('trunk', 'policy', 'value'):
        assert eng.tables[m].entries == off.tables[m].entries
    assert eng.params_total == off.params_total and eng.grads_total == off.grads_total


def test_invalid_row_count_rejected_at_create():
    from carla_driving_rl_agent_amd import _lib
    with pytest.raises(_lib.CdrlError, match='train_stats'):
        _engine(train_stats=-1)


def test_config_default_is_off():
    import ctypes as C
    from carla_driving_rl_agent_amd import _lib
    cfg = _lib.Config()
    cfg.train_stats = 7
    _lib.load().cdrl_config_default(C.byref(cfg))
    assert cfg.train_stats == 0


@pytest.mark.parametrize('written,rows,want', [(0, 4, []), (3, 4, [0, 1, 2]), (4, 4, [0, 1, 2, 3]), (7, 4, [3, 0, 1, 2]),
                                               (9, 4, [1, 2, 3, 0])])
def test_ring_order(written, rows, want):
    from carla_driving_rl_agent_amd import train_stats as ts
    assert ts.row_order(written, rows) == want


def test_decode_synthetic_block():
    """A block filled by hand through the reported offsets decodes to the values put in, oldest row first after a wrap."""
    from carla_driving_rl_agent_amd import train_stats as ts
    eng = _engine(train_stats=3)
    L, names = eng.train_stats_layout, _names(eng)
    block = np.zeros(L['header'] + L['rows'] * L['width'], np.float32)
    words = block.view(np.int32)
    words[0], words[1] = 5, 2                       # five appends to three rows: two lost, rows 2, 3, 4 held at indices 2, 0, 1
    for seq in range(5):
        row = block[L['header'] + (seq % 3) * L['width']:][:L['width']]
        irow = row.view(np.int32)
        kind = seq % 2
        irow[L['kind']], irow[L['t_head']], irow[L['t_dynamics']] = kind, seq // 2 + 1, seq + 1
        row[L['lr']], row[L['speed']], row[L['similarity']] = 1e-3 * (seq + 1), 0.1 * seq, -0.1 * seq
        row[L['metrics']:L['metrics'] + 16] = np.arange(16) + 100 * seq
        row[L['norms']:L['norms'] + 16] = np.arange(16) + 0.5
        row[L['trunk_norms']:L['trunk_norms'] + L['n_trunk']] = np.arange(L['n_trunk']) + 1000 * seq
    out = ts.decode(block, L, names)
    assert out['dropped'] == 2 and [r['t_dynamics'] for r in out['rows']] == [3, 4, 5]
    assert [r['kind'] for r in out['rows']] == ['policy', 'value', 'policy']
    r = out['rows'][1]
    assert r['lr'] == float(np.float32(4e-3)) and r['metrics'] == dict(loss=300.0, value_loss=301.0, speed_loss=302.0, similarity_loss=303.0)
    assert list(r['norms']) == names['value'] and list(r['trunk_norms']) == names['trunk']
    assert r['trunk_norms'][names['trunk'][-1]] == 3000.0 + L['n_trunk'] - 1
    assert out['rows'][0]['metrics']['log_prob'] == 206.0
    with pytest.raises(ValueError):
        ts.decode(block[:-1], L, names)
