"""The attention kernels' float64 reference, a restatement of their host plan, and the table of named cases
that tests/test_attn_cpu.py checks without a GPU and tests/test_attn_gpu.py runs on one.

Nothing here imports the code under test except ``formula32_error``, which runs ``_attn._softmax_pool`` (the
reference's formula) on float32 copies to size the tolerances of the wide and long cases.

Layout of every case: dim 0 is the attended axis; query ``(G, M, D)``, key ``(T, G, 1, D)``, value
``(T, G, 1, Dv)``, score ``(T, G, M)``, mask ``(T, G, M)``: G groups of M rows sharing a key and value sequence.
"""
import functools

import numpy as np
import torch

# ----------------------------------------------------------------------------------------------------------
# the formula


def pool_ref(score, value, mask, dim):
    """softmax over ``dim`` of ``score`` (masked frames at -inf), then the sum over ``dim`` of
    ``a[..., None] * value``: float64 torch on the CPU, differentiable."""
    assert score.dtype == torch.float64 and value.dtype == torch.float64
    if mask is not None:
        score = torch.where(mask, score, torch.full_like(score, -float("inf")))
    m = score.max(dim, keepdim=True).values
    p = torch.exp(score - m)
    a = p / p.sum(dim, keepdim=True)  # (a row with no finite score: exp(-inf + inf) = NaN, as torch.softmax)
    return (a.unsqueeze(-1) * value).sum(dim)


def attend_ref(query, key, value, mask, dim, scale):
    """``pool_ref`` of the scores ``scale * sum_i query_i key_i`` (query broadcast along ``dim``)."""
    assert query.dtype == torch.float64 and key.dtype == torch.float64
    return pool_ref((query.unsqueeze(dim) * key).sum(-1) * scale, value, mask, dim)


def drop_rows(mask, gout, dead):
    """The variant without the rows ``dead`` (a bool array over (G, M)): they attend every frame and receive
    a zero upstream gradient, so they take part in no gradient (dP = delta = 0 gives dS = 0 and a * dout = 0)
    and get none; the caller sets their output to NaN."""
    mask, gout = mask.copy(), gout.copy()
    mask[:, dead] = True
    gout[dead] = 0.0
    return mask, gout


# ----------------------------------------------------------------------------------------------------------
# the plan

ROWS, FRAMES, COLS, THREADS, LDS_BYTES, ROWS_MAX_D, ROWS_GROUP = 8, 32, 1024, 256, 57344, 32, 16
KINDS = {"dot": 0, "dot_bwd": 1, "pool": 2, "pool_bwd": 3}


def plan_of(G, M, T, D, Dv, esz, kind):
    """What ``attn_plan`` decides for a shape.  This is a Python restatement of two static C functions,
    ``attn_rows_per_tile`` and ``attn_plan`` (pydrobert-pytorch_amd/csrc/attn.hip:599-639), kept equal to
    them by ``test_attn_cpu.py::test_plan_restatement_matches_the_library`` through ``ws_bytes``.  ``kind`` is
    a key of ``KINDS``; ``D`` is ignored on the pool route."""
    pool, bwd = kind.startswith("pool"), kind.endswith("bwd")
    R, D = G * M, 0 if pool else D
    cols = D + Dv if bwd else D
    rt = min(ROWS, M, LDS_BYTES // (cols * esz) if cols else ROWS)
    assert rt >= 1
    tiles = -(-M // rt)
    frame_tiles = -(-T // FRAMES)
    p = dict(rt=rt, tiles=tiles, last_rows=M - (tiles - 1) * rt, zcols=0, rows_form=0, rows_wgs=0,
             lds_bytes=rt * cols * esz)  # fmt: skip
    if bwd:
        p.update(splits=max(1, frame_tiles), span=FRAMES)
        p["ws_bytes"] = R * esz + (0 if pool or p["splits"] == 1 else p["splits"] * R * D * esz)
    elif M >= ROWS_GROUP and D <= ROWS_MAX_D and Dv <= ROWS_MAX_D:
        p.update(rows_form=16 if D <= 16 and Dv <= 16 else ROWS_MAX_D, rows_wgs=-(-R // THREADS), splits=1,
                 span=0, ws_bytes=0)  # fmt: skip
    else:
        p["zcols"] = -(-Dv // COLS)
        blocks = G * tiles * p["zcols"]
        splits = min(max(1, -(-1024 // blocks)), max(1, frame_tiles))
        p["span"] = max(1, -(-frame_tiles // splits)) * FRAMES
        p["splits"] = max(1, -(-T // p["span"]))
        p["ws_bytes"] = 0 if p["splits"] == 1 else p["splits"] * R * (Dv + 2) * esz
    p["last_span"] = T - (p["splits"] - 1) * p["span"] if p["span"] else T
    return p


# ----------------------------------------------------------------------------------------------------------
# masks: recipe -> (T, G, M) bool array, and what each recipe claims (checked from the mask alone)


def _random_mask(rng, T, G, M):
    mask = rng.random((T, G, M)) < 0.7
    g, m = np.meshgrid(np.arange(G), np.arange(M), indexing="ij")
    mask[(g + m) % T, g, m] = True  # (every row attends something)
    return mask


def _dead_row(G, M):
    return G // 2, M // 2


def make_mask(recipe, rng, T, G, M):
    t = np.arange(T).reshape(T, 1, 1)
    g = np.arange(G).reshape(1, G, 1)
    m = np.arange(M).reshape(1, 1, M)
    if recipe is None:
        return None
    if recipe == "random":
        return _random_mask(rng, T, G, M)
    if recipe == "causal":  # (a limit per row, different for every row of a group)
        return t < np.maximum(1, 1 + ((m + 1) * T - 1) // M - g % 3)
    if recipe == "first_tile":  # (a third of the rows attend nothing in frames 0-31)
        return ~(((g + m) % 3 == 0) & (t < 32))
    if recipe == "middle_tile":  # (no row attends frames 32-63)
        return np.broadcast_to((t < 32) | (t >= 64), (T, G, M)).copy()
    if recipe == "dead_row":
        mask = _random_mask(rng, T, G, M)
        mask[(slice(None),) + _dead_row(G, M)] = False
        return mask
    if recipe == "spans":  # (T = 100 in four spans of 32)
        mask = _random_mask(rng, T, G, M)
        mask[:32, 0, 0] = False
        mask[96:, 0, 1] = False
        mask[:, 1, 2] = False
        return mask
    if recipe == "stagger":  # (a length per group; below it every row skips its own frames)
        lens = np.maximum(2, T - 3 - 5 * g)
        return (t < lens) & (((t + m) % 4 != 0) | (t == 0))
    raise KeyError(recipe)


def check_mask(recipe, mask, T, G, M):
    """Asserts what the recipe is named for, from the mask alone; returns the all-masked rows (G, M)."""
    dead = ~mask.any(0) if mask is not None else np.zeros((G, M), bool)
    if recipe in (None, "random", "causal", "first_tile", "middle_tile", "stagger"):
        assert not dead.any(), "no all-masked row outside the cases named for one"
    if recipe == "random":
        assert T == 1 or not mask.all()
    if recipe == "causal":
        limits = mask.sum(0)
        assert (mask == (np.arange(T).reshape(T, 1, 1) < limits)).all(), "a prefix per row"
        for g in range(G):
            assert len(set(limits[g].tolist())) >= min(M, T // 2), \
                "every row of a group (so of a tile) has its own limit, while the frames allow it"
    if recipe == "first_tile":
        some = (np.arange(G)[:, None] + np.arange(M)[None, :]) % 3 == 0
        assert some.any() and not some.all() and T > 32
        assert not mask[:32][:, some].any() and mask[32:][:, some].any(0).all(), \
            "these rows attend nothing in frames 0-31 and something later"
        assert mask[:32][:, ~some].all(), "the other rows attend the first tile"
    if recipe == "middle_tile":
        assert T > 64 and not mask[32:64].any() and mask[:32].all() and mask[64:].all(), \
            "frames 32-63 are attended by no row, every other frame by all"
    if recipe == "dead_row":
        assert dead.sum() == 1 and dead[_dead_row(G, M)], "one row attends nothing"
    if recipe == "spans":
        assert (T, G, M) == (100, 2, 3)
        assert not mask[:32, 0, 0].any() and all(mask[a:b, 0, 0].any() for a, b in ((32, 64), (64, 96), (96, 100))), \
            "row (0, 0) attends nothing in span 0 and something in every later span"
        assert not mask[96:, 0, 1].any() and all(mask[a:a + 32, 0, 1].any() for a in (0, 32, 64)), \
            "row (0, 1) attends nothing in the last span and something in every earlier one"
        assert dead.sum() == 1 and dead[1, 2], "row (1, 2) attends nothing"
    if recipe == "stagger":
        lens = T - np.argmax(mask.any(2)[::-1], 0)  # one past the last frame some row of the group attends
        for g in range(G):
            assert 2 <= lens[g] < T and not mask[lens[g]:, g].any(), \
                "the group's last frames are attended by none of its rows"
            assert M >= 4 or not mask[4, g].any(), "a group of fewer than four rows has such frames earlier too"
            if M >= 4:
                assert mask[:lens[g], g].any(1).all(), "every earlier frame is attended by some row"
                assert len({mask[:, g, m].tobytes() for m in range(min(M, 4))}) == min(M, 4), "the rows differ"
                for t0 in range(0, lens[g] - 1, FRAMES):
                    tile = mask[t0:min(t0 + FRAMES, lens[g]), g]
                    assert (tile.any(1) & ~tile.all(1)).any(), \
                        "every 32-frame tile has a frame that some row attends and some row does not"
    return dead


# ----------------------------------------------------------------------------------------------------------
# cases

SUITE = {"float32": (2e-5, 1e-4), "float64": (1e-9, 1e-8)}  # (output, gradients): the suite's bounds
CASES = {}


def _case(name, test, route, dtype, G, M, T, D, Dv, mask=None, form=None, tol=None, **kw):
    """``form``: the plan form the case is named for, ``dict(fwd=dict(...), bwd=dict(...))`` of ``plan_of``
    keys.  ``tol``: bounds from the measuring rule (max(suite bound, 8 * err32), err32 the float32 formula's
    own error on these inputs), by tensor name: ``out``, ``q``, ``k``, ``v``, ``e``; the suite's elsewhere.
    ``kw``: profile (score trend along T), shift, bad (non-finite masked frames), neginf (scores at -inf),
    qstride, vbt (value broadcast along T), expand (key and value expanded by the caller), gscale."""
    assert name not in CASES, name
    c = dict(name=name, test=test, route=route, dtype=dtype, G=G, M=M, T=T, D=0 if route == "pool" else D, Dv=Dv,
             mask=mask, form=form or {}, tol=tol or {}, seed=len(CASES) + 1, profile=None, shift=0.0, bad=False,
             neginf=False, qstride=1, vbt=False, expand=False, gscale=1.0)  # fmt: skip
    assert set(kw) <= set(c), kw
    c.update(kw)
    c["measured"] = bool(tol) or max(c["D"], Dv, T) > 300 or test == "shift"
    if c["measured"] and dtype == "float32":
        # an upstream gradient of 16 keeps these cases' gradients (a softmax over tens of frames times a
        # 1 / sqrt(D) scale leaves about 1e-3) a hundred times above the suite's absolute bound
        c["gscale"] = 16.0
    CASES[name] = c


def _both(name, test, **kw):
    for dtype in ("float32", "float64"):
        _case("{}-{}".format(name, dtype[-2:]), test, dtype=dtype, **kw)


# test_forward_walks_several_tiles_per_workgroup: 1100 groups fill the chip, so one workgroup walks all of T
_WALK = dict(fwd=dict(splits=1, span=96, last_span=70, rows_form=0, rt=1, zcols=1))
for _route in ("dot", "pool"):
    for _prof, _mask in (("rising", None), ("falling", None), ("flat", None), (None, "first_tile"),
                         (None, "middle_tile"), (None, "dead_row")):  # fmt: skip
        _both("walk-{}-{}".format(_route, _prof or _mask), "walk", route=_route, G=1100, M=1, T=70, D=20, Dv=20,
              mask=_mask, profile=_prof, form=_WALK)  # fmt: skip
    _both("walk-{}-carry-and-combine".format(_route), "walk", route=_route, G=300, M=1, T=250, D=20, Dv=20,
          mask="random", profile="rising", form=dict(fwd=dict(splits=4, span=64, last_span=58, rows_form=0)))
_case("walk-dot-control-one-tile-per-span", "walk", "dot", "float32", 130, 9, 100, 20, 20, "random",
      dict(fwd=dict(splits=4, span=32, rt=8, tiles=2, last_rows=1)))

# test_rows_per_tile_set_by_lds
_case("lds-fwd-rt7-32", "lds", "dot", "float32", 2, 9, 40, 1800, 8, "causal",
      dict(fwd=dict(rt=7, tiles=2, last_rows=2, lds_bytes=50400)))
_case("lds-fwd-rt1-64", "lds", "dot", "float64", 2, 3, 40, 3600, 8, "causal",
      dict(fwd=dict(rt=1, tiles=3, last_rows=1, lds_bytes=28800)))
_case("lds-bwd-rt7-32", "lds", "dot", "float32", 2, 9, 40, 1000, 1000, "causal",
      dict(fwd=dict(rt=8, tiles=2), bwd=dict(rt=7, tiles=2, last_rows=2, lds_bytes=56000)))
_case("lds-bwd-rt3-64", "lds", "dot", "float64", 2, 9, 40, 900, 900, "causal",
      dict(fwd=dict(rt=7, tiles=2), bwd=dict(rt=3, tiles=3, last_rows=3, lds_bytes=43200)))
_case("lds-pool-bwd-rt7-64", "lds", "pool", "float64", 2, 9, 40, 0, 1000, "causal",
      dict(fwd=dict(rt=8, tiles=2, lds_bytes=0), bwd=dict(rt=7, tiles=2, last_rows=2, lds_bytes=56000)))

# test_value_column_blocks: zcols 1 / 2 / 2 / 3 with split T, then zcols 2 unsplit
for _i, (_dt, _route, _Dv, _D, _T, _M, _z) in enumerate((
        ("float32", "dot", 1024, 5, 33, 1, 1), ("float64", "pool", 1024, 0, 70, 3, 1),
        ("float32", "pool", 1025, 0, 100, 2, 2), ("float64", "dot", 1025, 65, 33, 3, 2),
        ("float32", "dot", 1300, 257, 70, 3, 2), ("float64", "pool", 1300, 0, 33, 2, 2),
        ("float32", "dot", 2049, 65, 100, 2, 3), ("float64", "dot", 2049, 5, 70, 1, 3))):  # fmt: skip
    _case("cols-{}-{}-{}".format(_Dv, _route, _dt[-2:]), "cols", _route, _dt, 2, _M, _T, _D, _Dv, "random",
          dict(fwd=dict(zcols=_z, splits=-(-_T // 32), span=32)), dict(q=1.1e-4) if (_Dv, _dt) == (1024, "float32") else None)
_case("cols-1300-unsplit", "cols", "dot", "float32", 600, 1, 2, 5, 1300, None, dict(fwd=dict(zcols=2, splits=1)),
      dict(q=8.8e-4, k=7.7e-4))

# test_key_loop_tails: the forward strides D by 256 (four loads of 64), the backward by 64
for _D in (1, 63, 64, 65, 255, 256, 257, 300, 513):
    _both("keys-{}".format(_D), "keys", route="dot", G=2, M=3, T=33, D=_D, Dv=7, mask="random",
          form=dict(fwd=dict(rows_form=0, splits=2), bwd=dict(splits=2)))

# test_rows_kernel_forms
_both("rows-600-dead-row", "rows", route="dot", G=2, M=300, T=100, D=16, Dv=16, mask="dead_row",
      form=dict(fwd=dict(rows_form=16, rows_wgs=3)))
_both("rows-600-pool-17", "rows", route="pool", G=2, M=300, T=40, D=0, Dv=17, mask="causal",
      form=dict(fwd=dict(rows_form=32, rows_wgs=3)))
_both("rows-threshold-16-17-strided", "rows", route="dot", G=40, M=16, T=40, D=16, Dv=17, mask="random",
      qstride=2, form=dict(fwd=dict(rows_form=32, rows_wgs=3)))
_both("rows-32-32", "rows", route="dot", G=40, M=16, T=40, D=32, Dv=32, mask="causal",
      form=dict(fwd=dict(rows_form=32)))
_both("rows-pool-32", "rows", route="pool", G=40, M=16, T=40, D=0, Dv=32, mask="random",
      form=dict(fwd=dict(rows_form=32)))
_both("rows-1-1", "rows", route="dot", G=3, M=16, T=40, D=1, Dv=1, form=dict(fwd=dict(rows_form=16, rows_wgs=1)))
_both("rows-control-15", "rows", route="dot", G=40, M=15, T=40, D=16, Dv=16, mask="random",
      form=dict(fwd=dict(rows_form=0, rt=8, tiles=2, last_rows=7)))
_both("rows-control-33-8", "rows", route="dot", G=40, M=16, T=40, D=33, Dv=8, mask="random",
      form=dict(fwd=dict(rows_form=0, rt=8, tiles=2, last_rows=8)))
_both("rows-long-2000", "rows", route="dot", G=4, M=16, T=2000, D=16, Dv=16, mask="random",
      form=dict(fwd=dict(rows_form=16, rows_wgs=1)))

# test_backward_frame_chunk_forms: T <= 32 writes dQ directly, longer T goes through the dQ combine;
# R = 1, 3, 5 leave the delta kernel's last workgroup partial
for _i, (_T, _M, _G, _route) in enumerate(((1, 1, 1, "dot"), (31, 8, 2, "pool"), (32, 9, 1, "dot"),
                                           (32, 1, 3, "pool"), (33, 17, 1, "pool"), (33, 9, 2, "dot"),
                                           (64, 1, 3, "dot"), (64, 8, 1, "pool"), (65, 1, 5, "pool"),
                                           (65, 17, 1, "dot"), (31, 1, 5, "dot"))):  # fmt: skip
    _case("chunks-T{}-M{}-G{}-{}".format(_T, _M, _G, _route), "chunks", _route, ("float64", "float32")[_i % 2], _G,
          _M, _T, 6, 5, ("random", None, "causal")[_i % 3],
          dict(bwd=dict(splits=-(-_T // 32), rt=min(_M, 8), tiles=-(-_M // 8))))
_case("chunks-value-broadcast-along-T", "chunks", "dot", "float64", 2, 3, 65, 6, 5, "random",
      dict(bwd=dict(splits=3)), vbt=True)
_case("chunks-key-and-value-expanded", "chunks", "dot", "float64", 2, 3, 33, 6, 5, "random",
      dict(bwd=dict(splits=2, rt=1, tiles=1)), expand=True)
_case("chunks-pool-value-expanded", "chunks", "pool", "float32", 2, 3, 32, 0, 5, "random",
      dict(bwd=dict(splits=1, rt=1, tiles=1)), expand=True)

# test_split_partials_with_empty_spans
_SPANS = dict(fwd=dict(splits=4, span=32, last_span=4, rt=3), bwd=dict(splits=4))
_both("spans-dot", "spans", route="dot", G=2, M=3, T=100, D=6, Dv=5, mask="spans", form=_SPANS)
_both("spans-pool", "spans", route="pool", G=2, M=3, T=100, D=0, Dv=5, mask="spans", form=_SPANS)

# test_masked_non_finite_frames_in_every_route
_case("bad-group-of-9", "bad", "dot", "float32", 2, 9, 40, 6, 5, "stagger",
      dict(fwd=dict(splits=2, span=32, rt=8, tiles=2)), bad=True)
_case("bad-rows-kernel", "bad", "dot", "float32", 2, 16, 40, 8, 5, "stagger", dict(fwd=dict(rows_form=16)), bad=True)
_case("bad-pool-score-too", "bad", "pool", "float64", 2, 9, 40, 0, 5, "stagger",
      dict(fwd=dict(splits=2, rt=8, tiles=2)), bad=True)
_case("bad-pool-rows-kernel", "bad", "pool", "float32", 2, 16, 40, 0, 5, "stagger", dict(fwd=dict(rows_form=16)),
      bad=True)
_case("bad-unsplit", "bad", "dot", "float64", 2, 9, 20, 6, 5, "stagger", dict(fwd=dict(splits=1, span=32)), bad=True)
_case("bad-long-span", "bad", "dot", "float32", 1100, 1, 70, 6, 5, "stagger", dict(fwd=dict(splits=1, span=96)),
      bad=True)
_case("bad-long-span-pool", "bad", "pool", "float32", 1100, 1, 70, 0, 5, "stagger",
      dict(fwd=dict(splits=1, span=96)), bad=True)

# test_pool_scores_at_minus_infinity
_both("neginf-tiles", "neginf", route="pool", G=2, M=3, T=70, D=0, Dv=5, neginf=True,
      form=dict(fwd=dict(rows_form=0, splits=3)))
_both("neginf-tiles-unsplit", "neginf", route="pool", G=1100, M=1, T=70, D=0, Dv=5, neginf=True, mask="random",
      form=dict(fwd=dict(rows_form=0, splits=1, span=96)))
_both("neginf-rows", "neginf", route="pool", G=2, M=16, T=40, D=0, Dv=8, neginf=True, mask="random",
      form=dict(fwd=dict(rows_form=16)))

# test_all_masked_row_leaves_its_group_alone
_case("dead-9-dot", "dead", "dot", "float32", 2, 9, 40, 6, 5, "dead_row", dict(fwd=dict(rows_form=0, tiles=2)))
_case("dead-9-pool", "dead", "pool", "float64", 2, 9, 40, 0, 5, "dead_row", dict(fwd=dict(rows_form=0, tiles=2)))
_case("dead-70-dot", "dead", "dot", "float64", 2, 70, 40, 6, 5, "dead_row",
      dict(fwd=dict(rows_form=16), bwd=dict(tiles=9, last_rows=6)))
_case("dead-70-pool", "dead", "pool", "float32", 2, 70, 40, 0, 5, "dead_row",
      dict(fwd=dict(rows_form=16), bwd=dict(tiles=9, last_rows=6)))

# test_shifted_scores: the backward rebuilds a = exp(score - lse) from one stored float
_SHIFT_TOL = {  # 8 x err32: the float32 formula itself loses the low bits of a score near 100
    ("tiles", 10): dict(q=2.7e-4, k=1.3e-4), ("rows", 10): dict(q=1.1e-3, k=3.1e-4),
    ("tiles", 100): dict(out=4.1e-5, q=3.2e-3, k=1.3e-3, v=2.8e-4),
    ("rows", 100): dict(out=3.4e-5, q=4.5e-3, k=1.7e-3, v=3.8e-4),
}
for _s in (0, 10, 100):
    _case("shift-{}-tiles".format(_s), "shift", "dot", "float32", 2, 3, 70, 20, 20, None,
          dict(fwd=dict(rows_form=0, splits=3)), _SHIFT_TOL.get(("tiles", _s)), shift=float(_s), gscale=16.0)
    _case("shift-{}-rows".format(_s), "shift", "dot", "float32", 2, 16, 70, 16, 16, None,
          dict(fwd=dict(rows_form=16)), _SHIFT_TOL.get(("rows", _s)), shift=float(_s), gscale=16.0)


# Shapes for the plan alone (no tensors): enough groups that the row tiles per group, so the rows per tile
# that LDS allows at this element size, decide the number of spans: (G, M, T, D, Dv, esz, forward plan).
PLAN_ONLY = (
    (170, 16, 100, 1800, 8, 4, dict(rt=7, tiles=3, splits=2, span=64)),
    (170, 9, 100, 3600, 8, 4, dict(rt=3, tiles=3, splits=2, span=64)),
    (170, 3, 100, 3600, 8, 8, dict(rt=1, tiles=3, splits=2, span=64)),
    (200, 9, 200, 1800, 8, 8, dict(rt=3, tiles=3, splits=2, span=128)),
)


def cases_of(test):
    return [n for n, c in CASES.items() if c["test"] == test]


def plan_shape(c):
    """(G, M) as the plan sees them: a key and value the caller expanded leave groups of one row."""
    return (c["G"] * c["M"], 1) if c["expand"] else (c["G"], c["M"])


# ----------------------------------------------------------------------------------------------------------
# inputs (float64 numpy, rounded to the case's dtype so every precision sees the same numbers)


def _profile(name, T, flat=-1.0e4):
    t = np.arange(T, dtype=np.float64)
    return {"rising": 24.0 * t / T, "falling": -24.0 * t / T, "flat": np.full(T, flat)}[name]


def flat_score(c):
    """The flat profile's constant: -1e4, but -100 on the float32 dot route, where dQ = sum_t dS_t key_t has
    an error of |key| x the rounding of sum_t dS_t = 0 in any summation order: 1e-3 at 1e4, the suite's bound
    needs |key| of the order of 100."""
    return -100.0 if (c["route"], c["dtype"]) == ("dot", "float32") else -1.0e4


@functools.lru_cache(maxsize=None)
def build_inputs(name):
    """dict of float64 arrays ``q`` (G, M, D * qstride), ``k``, ``v``, ``e``, ``gout`` (G, M, Dv), the bool
    ``mask`` (or None), ``dead`` (G, M), ``scale``, and for the cases with non-finite masked frames the
    spoiled copies ``k_bad``, ``v_bad``, ``e_bad``.  Cached: treat as read-only."""
    c = CASES[name]
    G, M, T, D, Dv = c["G"], c["M"], c["T"], c["D"], c["Dv"]
    rng = np.random.default_rng(c["seed"])
    np_dt = np.float32 if c["dtype"] == "float32" else np.float64
    steer = c["profile"] is not None or c["shift"] > 0  # (feature 0 carries the trend: query 1 there)
    x = dict(scale=1.0 if steer or c["route"] == "pool" else float(D) ** -0.5)
    x["mask"] = make_mask(c["mask"], rng, T, G, M)
    x["dead"] = ~x["mask"].any(0) if x["mask"] is not None else np.zeros((G, M), bool)
    x["v"] = rng.normal(size=(1 if c["vbt"] else T, G, 1, Dv))
    x["gout"] = rng.normal(size=(G, M, Dv)) * c["gscale"]
    if c["route"] == "dot":
        q = rng.normal(size=(G, M, D, c["qstride"]))
        k = rng.normal(size=(T, G, 1, D))
        if steer:
            k *= 0.3 if c["profile"] is None else 0.05  # (the trend decides each tile's maximum)
            q[:, :, 0] = 1.0
            k[..., 0] = c["shift"]
            if c["profile"] is not None:
                k[..., 0] += _profile(c["profile"], T, flat_score(c)).reshape(T, 1, 1)
            if c["profile"] == "flat":
                k[..., 1:] = 0.0  # (every score of a row is the constant exactly)
        x["q"], x["k"] = q.reshape(G, M, D * c["qstride"]), k
    else:
        e = rng.normal(size=(T, G, M))
        if c["profile"] is not None:
            e = e * (0.0 if c["profile"] == "flat" else 0.2) + _profile(c["profile"], T).reshape(T, 1, 1)
        if c["neginf"]:
            e[rng.random((T, G, M)) < 0.2] = -np.inf
            g, m = np.meshgrid(np.arange(G), np.arange(M), indexing="ij")
            t = (g + m) % T  # (the frame every row's mask keeps: the row has a finite score)
            e[t, g, m] = np.where(np.isfinite(e[t, g, m]), e[t, g, m], 0.5)
        x["e"] = e
    for n in ("q", "k", "v", "e", "gout"):
        if n in x:
            x[n] = x[n].astype(np_dt).astype(np.float64)
    if c["bad"]:
        unseen = ~x["mask"].any(2)  # (T, G): frames no row of the group attends
        x["v_bad"] = x["v"].copy()
        x["v_bad"][unseen] = np.nan
        if c["route"] == "dot":
            x["k_bad"] = x["k"].copy()
            x["k_bad"][unseen] = np.inf
        else:
            x["e_bad"] = np.where(x["mask"], x["e"], np.where(np.arange(T).reshape(T, 1, 1) % 2, np.inf, np.nan))
    for a in x.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return x


def scores_of(name):
    """The case's scores (T, G, M) in float64, before the mask."""
    c, x = CASES[name], build_inputs(name)
    if c["route"] == "pool":
        return x["e"]
    return np.einsum("gmd,tgd->tgm", x["q"][..., ::c["qstride"]], x["k"][:, :, 0]) * x["scale"]


LEAVES = {"dot": ("q", "k", "v"), "pool": ("e", "v")}


def run_case(name, dot, pool, dtype, device, spoiled=False, dropped=True):
    """The case's forward and backward through the callables ``dot(query, key, value, mask, dim, scale)`` and
    ``pool(score, value, mask, dim)``: (out, {leaf name: gradient}).  With ``dropped`` an all-masked row is
    dropped as ``drop_rows`` describes (what a formula needs to have gradients at all); the kernels run with
    the mask as it is.  ``spoiled`` takes the non-finite copies of the inputs."""
    c, x = CASES[name], build_inputs(name)
    G, M, T, Dv = c["G"], c["M"], c["T"], c["Dv"]
    mask, gout = x["mask"], x["gout"]
    if dropped and x["dead"].any():
        mask, gout = drop_rows(mask, gout, x["dead"])
    L = {}
    for n in LEAVES[c["route"]]:
        a = x[n + "_bad"] if spoiled and n + "_bad" in x else x[n]
        L[n] = torch.from_numpy(a.copy()).to(device=device, dtype=dtype).requires_grad_(True)
    mask_t = None if mask is None else torch.from_numpy(mask.copy()).to(device)
    value = L["v"].expand(T, G, M, Dv) if c["expand"] else L["v"]
    if c["route"] == "dot":
        key = L["k"].expand(T, G, M, c["D"]) if c["expand"] else L["k"]
        out = dot(L["q"][..., ::c["qstride"]], key, value, mask_t, 0, x["scale"])
    else:
        out = pool(L["e"], value, mask_t, 0)
    names = list(L)
    grads = torch.autograd.grad(out, [L[n] for n in names], torch.from_numpy(gout.copy()).to(device=device, dtype=dtype))
    return out.detach(), dict(zip(names, (g.detach() for g in grads)))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The float64 reference of a case: (out, gradients), the all-masked rows' output NaN and the gradients
    those of the same rows without them.  Cached: treat as read-only."""
    out, grads = run_case(name, attend_ref, pool_ref, torch.float64, "cpu")
    dead = torch.from_numpy(build_inputs(name)["dead"].copy())
    out[dead] = float("nan")
    return out, grads


def formula32_error(name):
    """err32 by tensor name: the largest absolute error of the float32 formula on the CPU
    (``_attn._softmax_pool`` on float32 copies of the case's inputs) against ``expected``."""
    from pydrobert_amd._attn import _softmax_pool

    def dot(query, key, value, mask, dim, scale):
        return _softmax_pool((query.unsqueeze(dim) * key).sum(-1) * scale, value, mask, dim)

    out, grads = run_case(name, dot, _softmax_pool, torch.float32, "cpu")
    ref_out, ref_grads = expected(name)
    ok = ~torch.isnan(ref_out)
    err = {"out": float((out.double() - ref_out)[ok].abs().max())}
    for n, g in grads.items():
        err[n] = float((g.double() - ref_grads[n]).abs().max())
    return err


def bound(name, tensor):
    """(rtol, atol) of a tensor of a case: the suite's bound, or the case's measured one as atol."""
    c = CASES[name]
    suite = SUITE[c["dtype"]][0 if tensor == "out" else 1]
    return suite, c["tol"].get(tensor, suite)


def compare(name, out, grads, log=print):
    """Output, NaN pattern and every gradient of a run against ``expected``, each within ``bound``; an
    all-masked row's own gradient exactly 0 and every gradient finite.  Prints each figure first."""
    c, x = CASES[name], build_inputs(name)
    ref_out, ref_grads = expected(name)
    out = out.double().cpu()
    ok = ~torch.isnan(ref_out)
    assert out.shape == ref_out.shape
    assert torch.equal(torch.isnan(out), ~ok), "NaN exactly in the all-masked rows"
    failures = []
    for n, got, ref in [("out", out[ok], ref_out[ok])] + [(n, grads[n].double().cpu(), ref_grads[n]) for n in ref_grads]:
        rtol, atol = bound(name, n)
        assert got.shape == ref.shape, n
        err = float((got - ref).abs().max()) if got.numel() else 0.0
        fine = bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())
        log("{} {}: max abs error {:.3e} (atol {:.1e}, rtol {:.1e}){}".format(name, n, err, atol, rtol, "" if fine else " FAIL"))
        if not fine:
            failures.append((n, err))
    assert not failures, (name, failures)
    dead = torch.from_numpy(x["dead"].copy())
    if bool(dead.any()):
        own = grads["q"][dead] if c["route"] == "dot" else grads["e"][:, dead]
        assert bool((own == 0).all()), "an all-masked row's own gradient is exactly 0"
