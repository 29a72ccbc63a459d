"""Container of the full learner state: what `LearnerEngine.export_state()` returns plus the host-side counters and generators
of an agent, on disk under an agent's `base_path`.

    learner_state.index / .data-0000N-of-00002      the float32 arrays (params, adam_m, adam_v arenas; the three Nadam m_caches)
                                                    through this package's checkpoint-V2 codec (tf_checkpoint.py): crc32c per
                                                    tensor, temporary file + rename
    learner_state.json                              everything else: format version, manifest (optimizer, polyak, parameter
                                                    tables), step counters, Philox offsets, generator states
    learner_state.rank<r>.json                      data parallelism: rank r's own counters and generators

float32 arrays travel as bytes (NaN payloads, -0.0 and denormals come back bit for bit); integers -- the 128-bit PCG64 state
included -- travel as JSON integers, which Python keeps exact.

A state is complete or absent.  The JSON file is written last and names the checkpoint files it belongs to.  Successive saves
alternate between two file stems (`learner_state` and `learner_state.alt`), so the checkpoint files the current JSON names are never
written to: a save that fails at any point, the last rename included, leaves the previous complete state readable, and a first
save that fails leaves no JSON, which `load` refuses as incomplete.
"""
import json
import os
from typing import Dict, Optional, Tuple

import numpy as np

from . import tf_checkpoint

FORMAT_VERSION = 1
STEM = 'learner_state'
_STEMS = (STEM, STEM + '.alt')
_KEY = 'learner_state/'              # checkpoint keys: `learner_state/<array name>`


class LearnerStateError(RuntimeError):
    pass


def json_path(base_path: str) -> str:
    return os.path.join(base_path, STEM + '.json')


def rank_json_path(base_path: str, rank: int) -> str:
    return os.path.join(base_path, f'{STEM}.rank{int(rank)}.json')


def exists(base_path: str) -> bool:
    """Whether a complete state sits under `base_path` (its JSON file is there: it is written last)."""
    return os.path.exists(json_path(base_path))


def _write_json(path: str, obj: dict):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f'{path}.tmp{os.getpid()}'
    try:
        with open(tmp, 'w') as f:
            json.dump(obj, f)
        os.replace(tmp, path)
    except BaseException:
        try:                            # no temporary file left behind by a failed write
            os.unlink(tmp)
        except OSError:
            pass
        raise


def _read_json(path: str) -> dict:
    with open(path, 'r') as f:
        obj = json.load(f)
    version = obj.get('version') if isinstance(obj, dict) else None
    if version != FORMAT_VERSION:
        raise LearnerStateError(f'{path}: format version {version!r} is not supported (this package reads version {FORMAT_VERSION})')
    return obj


def _current_stem(base_path: str) -> Optional[str]:
    try:
        with open(json_path(base_path), 'r') as f:
            stem = json.load(f).get('checkpoint')
        return stem if stem in _STEMS else None
    except (OSError, ValueError, AttributeError):
        return None


def save(base_path: str, arrays: Dict[str, np.ndarray], meta: dict):
    """Writes float32 `arrays` and the JSON-able `meta` as one state under `base_path`: checkpoint files first, into the stem the
    current JSON does not name, then the JSON."""
    for name, a in arrays.items():
        if np.asarray(a).dtype != np.float32:
            raise LearnerStateError(f'learner state array {name!r} is {np.asarray(a).dtype}, not float32')
    stem = _STEMS[1] if _current_stem(base_path) == _STEMS[0] else _STEMS[0]
    tf_checkpoint.save_checkpoint(os.path.join(base_path, stem), {_KEY + k: np.asarray(v) for k, v in arrays.items()},
                                  object_graph=b'')
    obj = dict(meta)
    obj.update(version=FORMAT_VERSION, checkpoint=stem, arrays={k: list(np.asarray(v).shape) for k, v in arrays.items()})
    _write_json(json_path(base_path), obj)


def load(base_path: str) -> Tuple[Dict[str, np.ndarray], dict]:
    """-> (arrays, meta) of the state under `base_path`.  LearnerStateError for an incomplete state (no JSON), an unknown format
    version, a missing or corrupt checkpoint file (crc32c per array) or an array the JSON lists and the checkpoint lacks."""
    path = json_path(base_path)
    if not os.path.exists(path):
        raise LearnerStateError(f'{path} is missing: the learner state under {base_path} is incomplete or absent')
    meta = _read_json(path)
    stem = meta.get('checkpoint')
    if stem not in _STEMS:
        raise LearnerStateError(f'{path}: names no checkpoint of this package ({stem!r})')
    prefix = os.path.join(base_path, stem)
    try:
        tensors = tf_checkpoint.load_checkpoint(prefix, verify=True)
    except (OSError, ValueError, KeyError, IndexError) as e:
        raise LearnerStateError(f'{prefix}: unreadable learner state checkpoint: {e}') from e
    arrays = {k[len(_KEY):]: v for k, v in tensors.items() if k.startswith(_KEY)}
    for name, shape in meta.get('arrays', {}).items():
        if name not in arrays or list(arrays[name].shape) != list(shape):
            raise LearnerStateError(f'{prefix}: array {name!r} of shape {tuple(shape)} is missing from the checkpoint')
    return arrays, meta


def save_rank(base_path: str, rank: int, meta: dict):
    """Rank `rank`'s own host state (data parallelism), next to the state the writer rank saves."""
    obj = dict(meta)
    obj.update(version=FORMAT_VERSION, rank=int(rank))
    _write_json(rank_json_path(base_path, rank), obj)


def load_rank(base_path: str, rank: int) -> Optional[dict]:
    """Rank `rank`'s host state, or None when that rank wrote none (the world size changed): the caller keeps its defaults."""
    path = rank_json_path(base_path, rank)
    if not os.path.exists(path):
        return None
    return _read_json(path)


# ---------------------------------------------------------------------------------------------- manifest
def make_manifest(optimizer: str, polyak: float, tables: dict) -> dict:
    """optimizer name, polyak coefficient and, per model, the parameter table as [name, shape, trainable, offset] rows (the form
    tests/test_planner_tables_host.py dumps)."""
    return dict(optimizer=str(optimizer), polyak=float(polyak),
                tables={m: [[e['name'], [int(d) for d in e['shape']], bool(e['trainable']), int(e['offset'])] for e in t.entries]
                        for m, t in tables.items()})


def manifest_difference(have: dict, want: dict) -> Optional[str]:
    """None when a state with manifest `have` fits an engine with manifest `want`; otherwise one sentence naming the first
    difference.  The optimizer decides what the slot arenas mean and the tables where every tensor lies; the polyak coefficient is
    recorded and not compared (a hyper-parameter, free to change between runs).  Batch size, compute mode, freeze_trunk and train_stats
    are not part of a manifest: the tables do not depend on them."""
    if have.get('optimizer') != want.get('optimizer'):
        return f"optimizer: the state was written by {have.get('optimizer')!r}, the engine runs {want.get('optimizer')!r}"
    ht, wt = have.get('tables', {}), want.get('tables', {})
    for m in ('trunk', 'policy', 'value'):
        a, b = ht.get(m), wt.get(m)
        if a is None or b is None:
            return f'parameter table of {m!r}: missing from the {"state" if a is None else "engine"}'
        for i, (ra, rb) in enumerate(zip(a, b)):
            ra, rb = [ra[0], list(ra[1]), bool(ra[2]), int(ra[3])], [rb[0], list(rb[1]), bool(rb[2]), int(rb[3])]
            if ra != rb:
                return f'parameter table of {m!r}, entry {i}: the state has {ra}, the engine {rb}'
        if len(a) != len(b):
            return f'parameter table of {m!r}: the state has {len(a)} entries, the engine {len(b)}'
    return None


# ---------------------------------------------------------------------------------------------- generators
def numpy_global_state() -> list:
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return [name, [int(k) for k in keys], int(pos), int(has_gauss), float(cached).hex()]


def set_numpy_global_state(state: list):
    name, keys, pos, has_gauss, cached = state
    np.random.set_state((name, np.asarray(keys, dtype=np.uint32), int(pos), int(has_gauss), float.fromhex(cached)))


def python_random_state(rnd) -> list:
    version, internal, gauss_next = rnd.getstate()
    return [version, list(internal), None if gauss_next is None else float(gauss_next).hex()]


def set_python_random_state(rnd, state: list):
    version, internal, gauss_next = state
    rnd.setstate((version, tuple(internal), None if gauss_next is None else float.fromhex(gauss_next)))
