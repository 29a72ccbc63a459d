"""Host side of CARLAgent.explain (occlusion saliency): the cell geometry, the row order of the occluded variants of
one observation, and the argument checks.  Pure Python: importable without a GPU."""

BASELINES = ('zero', 'mean')            # cdrl_occlusion_baseline's modes, in this order
UPSAMPLES = ('nearest', 'bilinear')     # cdrl_occlusion_maps' modes, in this order
MAX_CHUNK = 65535                       # rows of one cdrl_occlusion_rows launch (the row is the grid's y dimension)
MODALITIES = ('image', 'road', 'vehicle', 'navigation')     # the four rows behind the cell rows, in this order


def occlusion_cells(H: int, W: int, gh: int, gw: int) -> list:
    """The gh * gw cells of an H x W frame, row-major: cell (cy, cx) = (y0, y1, x0, x1) covers rows [y0, y1) and columns [x0, x1),
    y0 = (cy * H) // gh, y1 = ((cy + 1) * H) // gh, columns alike.  No cell is empty and the cells partition the frame."""
    H, W, gh, gw = int(H), int(W), int(gh), int(gw)
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f'grid ({gh}, {gw}) outside 1..{H} x 1..{W}')
    return [((cy * H) // gh, ((cy + 1) * H) // gh, (cx * W) // gw, ((cx + 1) * W) // gw) for cy in range(gh) for cx in range(gw)]


def occlusion_frames(T: int, per_frame: bool) -> int:
    """F: one set of cells per frame, or one for the whole stack (a cell is then occluded in all T frames at once)."""
    return int(T) if per_frame else 1


def occlusion_row_count(T: int, gh: int, gw: int, per_frame: bool, modalities: bool) -> int:
    """N = 1 + F * gh * gw + (4 if modalities): the observation, its cell rows, then image / road / vehicle / navigation rows."""
    return 1 + occlusion_frames(T, per_frame) * int(gh) * int(gw) + (4 if modalities else 0)


def score_names(num_actions: int) -> list:
    """The K = 2 + A score columns."""
    return ['kl', 'value'] + [f'mean_{a}' for a in range(int(num_actions))]


def check_arguments(image_shape, envs: int, grid, baseline, upsample, chunk, row):
    """The checks of CARLAgent.explain on an (E, T, H, W, 3) image batch -> (gh, gw, baseline mode or None for a given stack,
    upsample mode).  ValueError: a grid outside 1..H x 1..W, an unknown baseline or upsample name, a baseline of the wrong shape,
    chunk outside 1..MAX_CHUNK, row outside 0..E-1."""
    T, H, W = (int(x) for x in image_shape[-4:-1])
    try:
        gh, gw = (int(g) for g in grid)
    except (TypeError, ValueError):
        raise ValueError(f'explain: grid must be a pair (gh, gw), got {grid!r}') from None
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f'explain: grid ({gh}, {gw}) outside 1..{H} x 1..{W}')
    if isinstance(baseline, str):
        if baseline not in BASELINES:
            raise ValueError(f'explain: baseline {baseline!r}: one of {BASELINES} or a ({T}, {H}, {W}, 3) tensor')
        mode = BASELINES.index(baseline)
    else:
        shape = tuple(getattr(baseline, 'shape', ()))
        if shape != (T, H, W, 3):
            raise ValueError(f'explain: a baseline stack must be ({T}, {H}, {W}, 3), got {shape}')
        mode = None
    if upsample not in UPSAMPLES:
        raise ValueError(f'explain: upsample {upsample!r}: one of {UPSAMPLES}')
    if not 1 <= int(chunk) <= MAX_CHUNK:
        raise ValueError(f'explain: chunk = {chunk}: 1 to {MAX_CHUNK} rows per forward')
    if not 0 <= int(row) < int(envs):
        raise ValueError(f'explain: row {row} outside 0..{int(envs) - 1}')
    return gh, gw, mode, UPSAMPLES.index(upsample)
