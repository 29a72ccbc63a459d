"""Host side of the update diagnostics ("train stats", include/cdrl.h): decoding the device ring into rows, and turning rows into
the scalars the reference logs from inside update() (rl/agents/ppo.py:209-225; core/carla_agent.py:140,382,423-426,461,483-484).

Pure numpy: importable and testable without a GPU or the library.  The layout is whatever cdrl_learner_train_stats_layout
reported (a dict of its fields); nothing about a row is hard-coded here except the order of the two metrics blocks, which is
CDRL_BUF_METRICS_P / _V's (include/cdrl.h)."""
from typing import Dict, List, Optional, Sequence

import numpy as np

KINDS = ('policy', 'value')
# CDRL_BUF_METRICS_P / CDRL_BUF_METRICS_V, in order (LearnerEngine.metrics uses the same names)
METRICS = dict(policy=('loss', 'policy_loss', 'entropy', 'speed_loss', 'similarity_loss', 'ratio', 'log_prob'),
               value=('loss', 'value_loss', 'speed_loss', 'similarity_loss'))
# logged by PPOAgent.update itself, per minibatch, from the loss the pass returned (kept that way: same values, same count)
LOGGED_BY_UPDATE = ('loss_total', 'lr_policy', 'loss_value', 'lr_value')


def row_order(written: int, rows: int) -> List[int]:
    """Ring indices of the rows still held after `written` appends to a ring of `rows`, oldest first."""
    if written <= rows:
        return list(range(written))
    return [(written + i) % rows for i in range(rows)]


def decode(block: np.ndarray, layout: Dict[str, int], names: Dict[str, Sequence[str]]) -> dict:
    """`block`: the ring as copied from the device (float32: header words then rows).  `names`: tensor names per model
    ('policy', 'value', 'trunk'; trainable tensors in parameter-table order).  -> dict(rows=[...oldest first], dropped=int); a row
    is dict(kind, t_head, t_dynamics, lr, lr_dynamics, clip_ratio, entropy_coef, speed, similarity, metrics={...},
    norms={name: float}, trunk_norms={name: float})."""
    block = np.ascontiguousarray(block, dtype=np.float32)
    L = layout
    if block.size != L['header'] + L['rows'] * L['width']:
        raise ValueError(f"train-stats block of {block.size} floats, layout says {L['header']} + {L['rows']} x {L['width']}")
    words = block.view(np.int32)
    written, dropped = int(words[0]), int(words[1])
    table = block[L['header']:].reshape(L['rows'], L['width'])
    out = []
    for r in row_order(written, L['rows']):
        row, irow = table[r], table[r].view(np.int32)
        kind = KINDS[int(irow[L['kind']])]
        rec = dict(kind=kind, t_head=int(irow[L['t_head']]), t_dynamics=int(irow[L['t_dynamics']]))
        for k in ('lr', 'lr_dynamics', 'clip_ratio', 'entropy_coef', 'speed', 'similarity'):
            rec[k] = float(row[L[k]])
        rec['metrics'] = {k: float(row[L['metrics'] + i]) for i, k in enumerate(METRICS[kind])}
        head = names[kind]
        if len(head) != L['n_' + kind] or len(names['trunk']) < L['n_trunk']:
            raise ValueError('train-stats layout and parameter table disagree on the tensor counts')
        rec['norms'] = {n: float(row[L['norms'] + i]) for i, n in enumerate(head)}
        rec['trunk_norms'] = {n: float(row[L['trunk_norms'] + i]) for i, n in enumerate(names['trunk'][:L['n_trunk']])}
        out.append(rec)
    return dict(rows=out, dropped=dropped)


def log_entries(rows: Sequence[dict], skip: Sequence[str] = ()) -> List[Dict[str, object]]:
    """One dict of `Agent.log(**kw)` keywords per row, under the reference's keys.  Loss keys against the reference's expressions:
    policy_objective logs speed_loss / similarity_loss WITH their factor 0.5 and entropy_penalty = entropy_coeff * entropy;
    value_objective logs the un-scaled value_loss as loss_v and its auxiliary terms without a factor, and returns
    0.25 * (their sum), which update() logs as loss_value.  `gradients_norm_*` are lists (one norm per tensor), as the reference
    logs them; the two dynamics keys are absent when the row carries no trunk norms (update_dynamics=False).  `skip`: keys to omit."""
    out = []
    for r in rows:
        m = r['metrics']
        if r['kind'] == 'policy':
            kw = dict(ratio=m['ratio'], log_prob=m['log_prob'], entropy=m['entropy'], entropy_coeff=r['entropy_coef'],
                      ratio_clip=r['clip_ratio'], loss_speed_policy=m['speed_loss'], loss_policy=m['policy_loss'],
                      loss_entropy=float(np.float32(r['entropy_coef']) * np.float32(m['entropy'])), speed_pi=r['speed'],
                      loss_similarity_policy=m['similarity_loss'], similarity_pi=r['similarity'])
            if r['trunk_norms']:
                kw['gradients_norm_dynamics'] = list(r['trunk_norms'].values())
            kw.update(loss_total=m['loss'], lr_policy=r['lr'], gradients_norm_policy=list(r['norms'].values()))
        else:
            kw = dict(speed_v=r['speed'], similarity_v=r['similarity'], loss_v=m['value_loss'], loss_speed_value=m['speed_loss'],
                      loss_similarity_value=m['similarity_loss'])
            if r['trunk_norms']:
                kw['gradients_norm_dynamics_v'] = list(r['trunk_norms'].values())
            kw.update(loss_value=m['loss'], lr_value=r['lr'], gradients_norm_value=list(r['norms'].values()))
        out.append({k: v for k, v in kw.items() if k not in skip})
    return out


def action_entries(actions) -> Optional[Dict[str, object]]:
    """CARLAgent.update's two action scalars (core/carla_agent.py:137-140): (actions - 1) * 2 + 1 of the memory's actions, column
    0 / column 1.  `actions`: (N, A) array or tensor; None when there are fewer than two columns (the reference prints a notice)."""
    if actions is None or len(actions.shape) != 2 or actions.shape[1] < 2:
        return None
    actions = (actions - 1.0) * 2.0 + 1.0
    return dict(action_throttle_or_brake=actions[:, 0], action_steer=actions[:, 1])
