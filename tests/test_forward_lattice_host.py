"""CPU: the case table of the forward sweep (tests/forward_lattice_cases.py) is the whole native space, recomputed here from
simnet.embedding_plan, and it reaches every split of the planner under every head dim the arithmetic allows."""
import forward_lattice_cases as cases


def _native_from_embedding_plan(vsa):
    native = set()
    for d in range(1, 1100):
        for H in range(1, d + 1):
            if d % H:
                continue
            try:
                plan = vsa.simnet.embedding_plan(d, H)
            except NotImplementedError:
                continue
            if plan is None:
                native.add((H, d))
    return native


def test_native_is_exactly_where_embedding_plan_returns_none(vsa):
    native = _native_from_embedding_plan(vsa)
    assert native == set(cases.NATIVE)
    assert len(cases.NATIVE) == len(set(cases.NATIVE)) == cases.NATIVE_COUNT == 44


def test_every_head_dim_on_every_side_of_d_model_256():
    """The planner splits at d_model <= 256 (bf16 storage), == 256 (the fused bf16 layer kernels) and > 256 (ring GEMMs): each
    head dim appears on every side it can - head dim 256 needs d_model >= 256, every other one divides 64, 256 and 512."""
    by_dh = {dh: sorted(d for H, d in cases.NATIVE if d // H == dh) for dh in cases.HEAD_DIMS}
    for dh, ds in by_dh.items():
        assert any(d < 256 for d in ds) == (dh < 256), dh
        assert any(d <= 256 for d in ds) and 256 in ds and any(d > 256 for d in ds), dh
    # the two shapes whose packed bf16 form asks for the bf16-stored head-dim-128 attention, and the wide one beside them
    assert {(2, 256), (1, 128), (4, 512)} <= set(cases.NATIVE)


def test_the_batch_straddles_the_tiles_and_the_latency_widths_straddle_the_slice_rule():
    L = cases.LENGTHS
    assert cases.ROWS == 421 and 1 in L and max(L) == 257
    for tile in (32, 128, 256):
        assert any(t < tile for t in L) and any(t > tile for t in L), tile
    assert cases.ROWS > 256                                     # above the fused bf16 kernels' default threshold
    eighths = [w // 8 for w in cases.LATENCY_IN_FEATURES]
    ok = [k % 128 == 0 and not (k > 256 and k % 256) for k in eighths]      # vsk_linear_parts_supported's slice rule
    assert ok == [True, True, False]
    assert all((H, d) in cases.NATIVE for H, d in cases.LATENCY_MODELS)
    assert sorted(d // H for H, d in cases.LATENCY_MODELS) == [32, 64, 128]
    assert len({cases.seeds(s) for s in cases.NATIVE}) == len(cases.NATIVE)
