"""Device-resident trace sets, host side (rl/trace_set.py): the code choice, the slot / lo tables, the epoch plan, the
bookkeeping and the refusals.  No GPU: the sets are built with upload=False."""
import os
import re

import numpy as np
import pytest

from carla_driving_rl_agent_amd import _lib, traces
from carla_driving_rl_agent_amd.rl import trace_set as TS
from tests import traceset_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, A = 4, 2
SPEC = dict(state_image=(6, 8, 3), state_road=(9,), state_vehicle=(12,), state_navigation=(11,))       # 28 slots: over 256 values each


def _spec(**kw):
    return TS.TraceSpec(SPEC, T, A, -1.0, 1.0, gamma=0.99, device='cpu', **kw)


def _trace(rng, n, stacked, info=True, reward=True, image=None):
    lead = (n, T) if stacked else (n,)
    states = dict(state_image=rng.integers(0, 256, lead + SPEC['state_image']).astype(np.float32) / np.float32(255.0) if image is None else image,
                  state_road=rng.integers(0, 2, lead + SPEC['state_road']).astype(np.float32),
                  state_vehicle=rng.standard_normal(lead + SPEC['state_vehicle']).astype(np.float16).astype(np.float32),
                  state_navigation=rng.random(lead + SPEC['state_navigation'], dtype=np.float32))
    return states, rng.uniform(-1, 1, (n, A)).astype(np.float32), rng.standard_normal(n + 1 if reward else n).astype(np.float32), \
        dict(speed=rng.uniform(0, 80, n), similarity=rng.uniform(-1, 1, n)) if info else None


def _write(path, episode, rng, n, stacked, **kw):
    states, actions, rewards, info = _trace(rng, n, stacked, **kw)
    if len(rewards) == n:       # a trace without usable returns: write_trace insists on rewards, so drop them afterwards
        file = traces.write_trace(path, episode, states, actions, rewards, np.zeros(n), info)
        with np.load(file) as f:
            kept = {k: f[k] for k in f.keys() if k != 'reward'}
        np.savez_compressed(file, **kept)
        return file
    return traces.write_trace(path, episode, states, actions, rewards, np.zeros(n), info)


@pytest.fixture(scope='module')
def mixed_dir(tmp_path_factory):
    """Per-step traces of 7 and 1 rows around a stacked one of 5: 13 rows, 7 + 20 + 1 slots."""
    path, rng = str(tmp_path_factory.mktemp('mixed')), np.random.default_rng(5)
    _write(path, 1, rng, 7, False)
    _write(path, 2, rng, 5, True)
    _write(path, 3, rng, 1, False)
    return path


# ---------------------------------------------------------------------------------------------------------------- the code choice
def test_exact_picks_the_smallest_lossless_code():
    rng = np.random.default_rng(0)
    camera = rng.integers(0, 256, (3, 40, 30)).astype(np.float32) / np.float32(255.0)
    for data, want in ((camera, 'u8'), (rng.integers(0, 256, (5, 77)).astype(np.float32) / np.float32(127.5) - np.float32(1.0), 'u8'),
                       (rng.integers(0, 2, (11, 9)).astype(np.float32), 'u8'),
                       (np.arange(257, dtype=np.float32).reshape(1, 257), 'f16'),            # 257 values: no palette; all are halves
                       (np.arange(257, dtype=np.float32).reshape(1, 257) + np.float32(0.1), 'f32'),
                       (rng.standard_normal((4, 999)).astype(np.float16).astype(np.float32), 'f16'),
                       (rng.random((4, 999), dtype=np.float32), 'f32')):
        code, parts, pal = TS.choose_code([data[:1], data[1:]])
        assert code == want
        assert (pal is not None) == (code == 'u8')
        back = np.concatenate([TS.decode(code, p, pal) for p in parts])
        assert np.array_equal(back, ref.bits(data))


def test_palette_keeps_the_two_zeros_and_nan_payloads_apart():
    data = np.array([0x00000000, 0x80000000, 0x7fc00000, 0x7fc00001, 0xffc00000, 0x3f800000, 0x80000000], np.uint32).view(np.float32)
    code, (coded,), pal = TS.choose_code([data.reshape(1, -1)])
    assert code == 'u8' and pal.shape == (256,) and pal.dtype == np.uint32
    assert len(set(coded.reshape(-1)[:6])) == 6 and coded[0, 1] == coded[0, 6]
    assert np.array_equal(TS.decode(code, coded, pal).reshape(-1), data.view(np.uint32))
    halves = np.concatenate([np.arange(300, dtype=np.float32), [-0.0, np.inf, -np.inf, 2.0 ** -24, -2.0 ** -20]]).astype(np.float32)
    code, (coded,), _ = TS.choose_code([halves.reshape(1, -1)])
    assert code == 'f16' and np.array_equal(TS.decode(code, coded), ref.bits(halves).reshape(1, -1))


def test_half_decoding_is_the_format_for_every_pattern():
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(TS.half_bits_to_float_bits(every), ref.half_to_float_bits(every))
    finite = (every & 0x7c00) != 0x7c00
    assert np.array_equal(TS.half_bits_to_float_bits(every)[finite], every.view(np.float16).astype(np.float32).view(np.uint32)[finite])
    assert np.array_equal(TS.encode_half(every.view(np.float16).astype(np.float32))[finite], every[finite])


def test_forced_half_is_the_only_lossy_choice():
    data = np.random.default_rng(1).random((3, 50), dtype=np.float32)
    code, (coded,), pal = TS.choose_code([data], force='f16')
    assert code == 'f16' and pal is None
    assert np.array_equal(TS.decode(code, coded), ref.bits(data.astype(np.float16).astype(np.float32)))
    with pytest.raises(ValueError, match='force'):
        TS.choose_code([data], force='u8')


# --------------------------------------------------------------------------------------------------------------------- the tables
def test_tables_window_per_step_traces_and_return_stacked_rows():
    layout = [(7, False), (5, True), (1, False)]
    slot, lo, first, slots = TS.build_tables(layout, T)
    rslot, rlo, rslots = ref.tables(layout, T)
    assert np.array_equal(slot, rslot) and np.array_equal(lo, rlo) and slots == rslots == 7 + 20 + 1 and first == [0, 7, 27]
    frames = np.maximum(slot[:, None] - (T - 1 - np.arange(T))[None, :], lo[:, None])
    assert np.array_equal(frames[:7], traces.window_index(7, T).reshape(7, T))                    # the first frame repeats
    assert np.array_equal(frames[7:12], 7 + np.arange(20).reshape(5, T))                          # its own T frames
    assert np.array_equal(frames[12], np.full(T, 27))                                             # a one-row trace
    assert slot.dtype == lo.dtype == np.int32


def test_a_set_from_a_mixed_directory(mixed_dir):
    ts = TS.TraceSet.from_dir(_spec(), mixed_dir, upload=False)
    assert (ts.rows, ts.traces, ts.slots, ts.T) == (13, 3, 28, T)
    assert ts.layout == [(7, False), (5, True), (1, False)] and [ts.trace_rows(i) for i in range(3)] == [(0, 7), (7, 5), (12, 1)]
    assert ts.codes == dict(state_image='u8', state_road='u8', state_vehicle='f16', state_navigation='f32')
    assert ts.has_info and ts.has_value and not ts.has_weight
    assert ts.column_ranges == dict(u=(0, 2), speed=(2, 3), similarity=(3, 4), returns=(4, 6)) and ts.width == 6
    loaded = list(traces.load_traces(mixed_dir))
    decoded = {k: TS.decode(ts.codes[k], ts.coded[k], ts.palettes[k]) for k in ts.codes}
    at = 0
    for trace, (n, stacked) in zip(loaded, ts.layout):
        for k in ts.codes:
            want = ref.bits(trace[k]).reshape(n * T if stacked else n, -1)
            assert np.array_equal(decoded[k][at:at + want.shape[0]], want), k
        at += n * T if stacked else n
    u = np.concatenate([traces.unit_actions(t['action'], -1.0, 1.0) for t in loaded])
    assert np.array_equal(ts.host_columns[:, :2], u)
    assert np.array_equal(ts.host_columns[:, 2], np.concatenate([t['info_speed'].reshape(-1) for t in loaded]))    # / 100 on the device
    nb = ts.nbytes
    assert nb['state_image'] == dict(code='u8', bytes=28 * 144) and nb['state_road'] == dict(code='u8', bytes=28 * 9)
    assert nb['state_vehicle'] == dict(code='f16', bytes=28 * 12 * 2) and nb['state_navigation'] == dict(code='f32', bytes=28 * 11 * 4)
    assert nb['palettes'] == 2048 and nb['tables'] == 8 * 13 and nb['columns'] == 4 * 13 * 6
    assert nb['total'] == 28 * (144 + 9 + 24 + 44) + 2048 + 104 + 312
    with pytest.raises(RuntimeError, match='upload=False'):
        ts.trace_tensors(0)


def test_columns_follow_what_every_trace_has(tmp_path):
    rng = np.random.default_rng(2)
    path = str(tmp_path / 'bare')
    _write(path, 1, rng, 4, False)
    _write(path, 2, rng, 3, False, info=False, reward=False)
    ts = TS.TraceSet.from_dir(_spec(), path, upload=False, weights=lambda t: np.arange(t['action'].shape[0]))
    assert not ts.has_info and not ts.has_value and ts.has_weight and ts.column_ranges == dict(u=(0, 2), weight=(2, 3))
    assert np.array_equal(ts.host_columns[:, 2], [0, 1, 2, 3, 0, 1, 2])
    assert TS.TraceSet.from_dir(_spec(), path, upload=False, max_traces=1).has_info
    with pytest.raises(ValueError, match=r'trace-2-.*weights\(trace\) returned 2 values for a trace of 3 rows'):
        TS.TraceSet.from_dir(_spec(), path, upload=False, weights=lambda t: np.zeros(2) if t['action'].shape[0] == 3 else np.zeros(4))


def test_storage_f16_halves_the_image_alone(mixed_dir):
    ts = TS.TraceSet.from_dir(_spec(), mixed_dir, upload=False, storage='f16')
    assert ts.codes == dict(state_image='f16', state_road='u8', state_vehicle='f16', state_navigation='f32')
    first = next(iter(traces.load_traces(mixed_dir)))
    assert np.array_equal(TS.decode('f16', ts.coded['state_image'][:7]),
                          ref.bits(first['state_image'].astype(np.float16).astype(np.float32)).reshape(7, -1))
    with pytest.raises(ValueError, match='storage'):
        TS.TraceSet.from_dir(_spec(), mixed_dir, upload=False, storage='bf16')


# ----------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_epoch_is_a_true_shuffle(mixed_dir):
    ts = TS.TraceSet.from_dir(_spec(), mixed_dir, upload=False)
    order, cuts = ts.plan_epoch(np.random.default_rng(9), 4)
    assert order.dtype == np.int32 and sorted(order) == list(range(13))                           # every row exactly once
    assert cuts == [(0, 4), (4, 4), (8, 4), (12, 1)]                                              # the ragged tail
    again, _ = ts.plan_epoch(np.random.default_rng(9), 4)
    other, _ = ts.plan_epoch(np.random.default_rng(10), 4)
    assert np.array_equal(order, again) and not np.array_equal(order, other)
    assert np.array_equal(order, np.random.default_rng(9).permutation(13))
    assert ts.plan_epoch(np.random.default_rng(9), 4, drop_remainder=True)[1] == [(0, 4), (4, 4), (8, 4)]
    assert ts.plan_epoch(np.random.default_rng(9), 50)[1] == [(0, 13)] and ts.plan_epoch(np.random.default_rng(9), 50, True)[1] == []
    assert ts.epoch_order(np.random.default_rng(3)) == list(np.random.default_rng(3).permutation(3))
    assert ts.epoch_order(np.random.default_rng(3), 2) == list(np.random.default_rng(3).permutation(3)[:2])
    with pytest.raises(ValueError, match='batch_size'):
        ts.plan_epoch(np.random.default_rng(9), 0)


# ------------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_name_the_file_and_the_key(tmp_path, mixed_dir):
    ts = TS.TraceSet.from_dir(_spec(), mixed_dir, upload=False)
    assert np.array_equal(ts.check_index([0, 12, 3, 3]), [0, 12, 3, 3]) and ts.check_index([0]).dtype == np.int32
    for bad in ([0, 13], [-1], [2 ** 31]):
        with pytest.raises(ValueError, match=r'outside 0\.\.12'):
            ts.check_index(bad)
    with pytest.raises(ValueError, match='1-D integer'):
        ts.check_index(np.zeros(3, np.float32))
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(ValueError, match='no trace-'):
        TS.TraceSet.from_dir(_spec(), str(empty), upload=False)
    rng = np.random.default_rng(4)
    odd = str(tmp_path / 'odd')
    _write(odd, 1, rng, 4, False)
    _write(odd, 2, rng, 4, False, image=np.zeros((4, 6, 9, 3), np.float32))
    with pytest.raises(ValueError, match=r'trace-2-.*state_image has shape \(4, 6, 9, 3\)'):
        TS.TraceSet.from_dir(_spec(), odd, upload=False)
    assert TS.TraceSet.from_dir(_spec(), odd, upload=False, max_traces=1).rows == 4
    with pytest.raises(ValueError, match='carries a time axis'):
        TS.TraceSet.from_dir(_spec(stacks_time=False), mixed_dir, upload=False)
    wide = TS.TraceSpec(SPEC, T, 3, -1.0, 1.0, device='cpu')
    with pytest.raises(ValueError, match='width 2'):
        TS.TraceSet.from_dir(wide, mixed_dir, upload=False)
    with pytest.raises(ValueError, match='load it with this agent'):
        ts.check_fits(wide)
    with pytest.raises(ValueError, match='load it with this agent'):
        ts.check_fits(TS.TraceSpec(dict(SPEC, state_road=(8,)), T, A, -1.0, 1.0, device='cpu'))
    ts.check_fits(_spec())


def test_header_binding_and_sources_agree():
    with open(os.path.join(ROOT, 'include', 'cdrl.h')) as f:
        header = f.read()
    assert re.search(r'^int cdrl_traceset_batch\(', header, re.M) and 'cdrl_traceset_batch' in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES['cdrl_traceset_batch'][1]) == 9
    for name, value in (('CDRL_TRACE_F32', _lib.TRACE_F32), ('CDRL_TRACE_F16', _lib.TRACE_F16), ('CDRL_TRACE_U8', _lib.TRACE_U8)):
        assert f'{name} = {value}' in header and value == getattr(ref, name[-3:].replace('_', ''))
    import ctypes as C
    assert C.sizeof(_lib.TraceSetKey) == 56
    with open(os.path.join(ROOT, 'carla-driving-rl-agent_amd', 'build.py')) as f:
        assert "'traceset'" in f.read()
