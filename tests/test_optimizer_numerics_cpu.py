"""The optimizer-numerics bounds (tests/optimizer_numerics.py) are neither
tight nor loose: (a) a torch fp32 emulation with the kernels' rounding points
- 16-entry chunk partials from +0, combined in ascending, reverse and random
order, one rounding to bf16; adam_update4 operation by operation in its FMA
and non-FMA lanes, and the scalar source with every operation rounded on its
own - passes every bound with zero violations at every shape of
test_optimizer_numerics_gpu.py; (b) mutations of the fp64 reference, each a
plausible kernel bug, are flagged at the planted elements.

No GPU.  Run with -s to see max |err| / tol per output.
"""

import pytest
import torch

import optimizer_numerics as N

bf16 = torch.bfloat16
f32 = torch.float32

ADAM_NS = (1, 4, 5, 1000, 1023, 4097, 9219, 37 * 104, 4096 * 256 + 77)
TS_ = (1, 2, 1000)
WDS = (0.0, 0.01)
MULTI_SIZES = (1, 3, 255, 256, 257, 1000, 4097, 5)
MULTI_GRID_STRIDE = (1, 3, 255, 256, 257, 1024, 7, 4096 * 256 + 100)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    N.print_worst("CPU emulation")


# ---------------------------------------------------------------------------
# planted data


@pytest.mark.parametrize("thr", N.THRS)
@pytest.mark.parametrize("plan", sorted(N.M_OF))
def test_plan_holds_every_planted_run(plan, thr):
    c = N.scatter_case(plan, thr, 8, 8)
    assert c.T % 64 and c.P % 64
    for tag, tb in c.tables.items():
        pos, nm = N.plan_positions(tb.plan), tb.named
        cnt = dict(tb.plan)
        assert (tb.N % 16 != 0) == (plan == "odd")
        rows = [r for r, _ in tb.plan]
        assert rows == sorted(rows) and len(set(rows)) == len(rows)
        assert torch.equal(torch.bincount(tb.idx.long(), minlength=tb.rows),
                           torch.tensor([cnt.get(r, 0)
                                         for r in range(tb.rows)]))
        assert pos[0][0] == 0 and (pos[0][1] + 1) % 16 != 0
        a, b = pos[nm["heavy"]]
        assert a % 16 and (b + 1) % 16 and tb.span[nm["heavy"]] >= 12
        assert cnt[nm["heavy"]] > max(N.THRS)
        a, b = pos[nm["fill16"]]
        assert a % 16 == 0 and b - a == 15
        a, b = pos[nm["r17"]]
        assert a % 16 == 0 and b - a == 16
        a, b = pos[nm["straddle"]]
        assert b - a == 1 and a % 16 == 15
        for key, n, aligned in (("thr_al", thr, True), ("thr1_al", thr + 1, True),
                                ("thr_un", thr, False),
                                ("thr1_un", thr + 1, False)):
            a, b = pos[nm[key]]
            assert b - a + 1 == n and (a % 16 == 0) == aligned
        a, b = pos[nm["r48"]]
        assert a % 16 == 0 and b - a == 47
        a, b = pos[nm["heavy_edge"]]
        assert a % 16 and (b + 1) % 16 == 0 and cnt[nm["heavy_edge"]] > 64
        assert cnt[nm["single_a"]] == cnt[nm["single_b"]] == 1
        assert nm["untouched"] not in cnt and nm["untouched"] == tb.rows - 2
        assert pos[nm["last"]][1] == tb.N - 1 and nm["last"] == tb.rows - 1
    # both halves feed every planted term-table run
    tb = c.tables["term"]
    for r, n in tb.plan[:17]:
        if n >= 2:
            assert bool((c.starts == r).any()) and bool((c.ends == r).any())
    g = N.d(c.gout)[:, :2 * c.TS + c.PS]
    nz = g[g != 0].abs()
    assert float(nz.min()) >= 0.5 and float(nz.max()) <= 2.0


# ---------------------------------------------------------------------------
# not tight: the emulation passes every bound


@pytest.mark.parametrize("key", N.all_scatter_keys(),
                         ids=lambda k: "-".join(map(str, k)))
def test_scatter_emulation_within_bounds(key):
    c = N.scatter_case(*key)
    for tag, tb in c.tables.items():
        ref, tol, _, _ = N.table_ref(c, tag)
        for order in ("ascending", "reverse", "random"):
            got = N.emu_scatter(tb, c.gout, order)
            N.within(got, ref, tol, f"table gradient ({tag})",
                     f"{c.name()} {order}")
            if c.grad == "int":
                assert torch.equal(got, ref.float().to(bf16))
            assert float(got[0].abs().sum()) == 0
            assert float(got[tb.named["untouched"]].abs().sum()) == 0


def _adam_emulated(n, t, wd, lane, grad_dtype=bf16):
    hp = N.Hyper(wd=wd)
    old = N.adam_state(n, grad_dtype)
    pw = hp.pow_at(t)
    new = N.emu_adam(old, old["g"], pw, hp, lane)
    return hp, old, pw, new


@pytest.mark.parametrize("wd", WDS)
@pytest.mark.parametrize("t", TS_)
def test_adam_emulation_within_bounds(t, wd):
    for n in ADAM_NS:
        for lane in ("fma", "nofma", "scalar"):
            hp, old, pw, new = _adam_emulated(n, t, wd, lane)
            N.adam_check(f"n={n} t={t} wd={wd} {lane}", old, new,
                         N.d(old["g"]), pw, hp, "adam emulation",
                         scalar_from=0 if lane == "scalar" else None)
            if wd == 0.0:
                # planted g = 0, m = v = 0: an exact no-op
                assert new["p"][0] == old["p"][0] and new["m"][0] == 0


@pytest.mark.parametrize("sizes", [MULTI_SIZES, MULTI_GRID_STRIDE],
                         ids=["small", "grid-stride"])
@pytest.mark.parametrize("t,wd", [(1, 0.0), (2, 0.01), (1000, 0.01)])
def test_adam_f32_multi_emulation_within_bounds(sizes, t, wd):
    hp = N.Hyper(wd=wd)
    states = [N.adam_state(n, f32, seed=i) for i, n in enumerate(sizes)]
    old = N.multi_concat(states)
    pw = hp.pow_at(t)
    new = N.emu_adam(old, old["g"], pw, hp, "scalar")
    del new["param"]
    N.adam_check(f"multi sizes={sizes[-3:]} t={t} wd={wd}", old, new,
                 N.d(old["g"]), pw, hp, "adam emulation", scalar_from=0)


@pytest.mark.parametrize("key", N.all_scatter_keys(),
                         ids=lambda k: "-".join(map(str, k)))
def test_table_adam_emulation_within_bounds(key):
    """K16b: scatter emulation -> bf16 gradient -> adam_update4 emulation,
    judged against the fp64 gradient with the dg-widened bounds."""
    c = N.scatter_case(*key)
    for tag, tb in c.tables.items():
        ref, tol, _, _ = N.table_ref(c, tag)
        g = N.emu_scatter(tb, c.gout, "random", seed=3)
        old = N.adam_state(tb.rows * tb.S, bf16, seed=11)
        for t, wd in ((1, 0.0), (2, 0.01), (1000, 0.01)):
            hp = N.Hyper(wd=wd)
            pw = hp.pow_at(t)
            for lane in ("fma", "nofma"):
                new = N.emu_adam(old, g.reshape(-1), pw, hp, lane)
                if c.grad == "int":
                    g64, dg = N.d(ref.float().to(bf16)), None
                else:
                    g64, dg = ref, tol
                N.adam_check(f"{c.name()} {tag} t={t} wd={wd} {lane}", old,
                             new, g64, pw, hp, "table adam emulation", dg=dg)


@pytest.mark.parametrize("mutation", ["drop_first", "drop_edge", "drop_chunk",
                                      "drop_tail", "ends_at_off0",
                                      "pad_summed", "drop_last_row"])
def test_table_adam_sees_a_mutated_gradient(mutation):
    """The dg-widened K16b bounds still flag a gradient that lost an entry:
    a lost entry costs 0.5, dg is about U |g|."""
    c = N.scatter_case("odd", 32, 136, 104, "padnz")
    tb = c.tables["term"]
    hp = N.Hyper(wd=0.01)
    pw = hp.pow_at(2)
    g = N.emu_scatter(tb, c.gout, "ascending")
    old = N.adam_state(tb.rows * tb.S, bf16, seed=11)
    new = N.emu_adam(old, g.reshape(-1), pw, hp, "fma")
    ref, tol, _, _ = N.table_ref(c, "term")
    assert N.adam_check("", old, new, ref, pw, hp, "emu", dg=tol,
                        count_only=True) == 0
    mref, mmag, n_r = N.table_grad_ref(tb, c.gout, mutation)
    assert N.adam_check("", old, new, mref, pw, hp, "emu",
                        dg=N.table_grad_tol(mref, mmag, n_r),
                        count_only=True) > 0


# ---------------------------------------------------------------------------
# not loose: mutated references are flagged


SCATTER_MUTATIONS = ("drop_first", "drop_last", "drop_edge", "drop_chunk",
                     "drop_head", "drop_tail", "ends_at_off0", "pad_summed",
                     "drop_last_row", "drop_cols128", "drop_tail_entries")


@pytest.mark.parametrize("mutation", SCATTER_MUTATIONS)
def test_scatter_mutations_are_flagged(mutation):
    c = N.scatter_case("odd", 32, 136, 104, "padnz")
    tb = c.tables["term"]
    got = N.emu_scatter(tb, c.gout, "ascending")
    ref, tol, _, _ = N.table_ref(c, "term")
    assert not bool(N.violations(got, ref, tol).any())
    mref, mmag, n_r = N.table_grad_ref(tb, c.gout, mutation)
    bad = N.violations(got, mref, N.table_grad_tol(mref, mmag, n_r))
    assert bool(bad.any()), mutation
    rows = set(torch.nonzero(bad.any(dim=1)).flatten().tolist())
    nm = tb.named
    want = {"drop_first": {nm["heavy"]}, "drop_last": {nm["r17"]},
            "drop_edge": {nm["heavy"]}, "drop_chunk": {nm["heavy"]},
            "drop_head": {nm["heavy"]}, "drop_tail": {nm["heavy"]},
            "pad_summed": {0}, "drop_last_row": {nm["last"]}}.get(mutation)
    if want is not None:
        assert rows == want, (mutation, sorted(rows))
    elif mutation == "ends_at_off0":
        # every touched row but PAD has an entry in the ends half or not;
        # all planted runs of two or more do
        assert {nm["heavy"], nm["straddle"], nm["last"]} <= rows
    elif mutation == "drop_cols128":
        cols = torch.nonzero(bad.any(dim=0)).flatten()
        assert int(cols.min()) == 128 and int(cols.max()) == tb.S - 1
        assert nm["heavy"] in rows and nm["single_a"] in rows
    else:  # the last N % 16 entries all belong to the last rows
        assert nm["last"] in rows


ADAM_MUTATIONS = ("no_wd", "bc_prev", "bc_swap", "eps_in_sqrt", "v_from_G",
                  "tail_skipped")


@pytest.mark.parametrize("mutation", ADAM_MUTATIONS)
def test_adam_mutations_are_flagged(mutation):
    n = 4097 if mutation != "tail_skipped" else 1023
    for lane in ("fma", "nofma"):
        hp, old, pw, new = _adam_emulated(n, 2, 0.01, lane)
        g64 = N.d(old["g"])
        assert N.adam_check("", old, new, g64, pw, hp, "emu",
                            count_only=True) == 0
        assert N.adam_check("", old, new, g64, pw, hp, "emu", mutate=mutation,
                            count_only=True) > 0, (mutation, lane)


def test_adam_eps_placement_shows_at_the_planted_element():
    """eps inside the square root is visible where eps dominates the
    denominator: the planted |g| = 1e-9, m = v = 0 elements."""
    hp, old, pw, new = _adam_emulated(4097, 1, 0.0, "fma")
    ref, tol = N.adam_param_ref(old, new["m"], new["v"], pw, hp,
                                "eps_in_sqrt")
    bad = N.violations(new["p"], ref, tol)
    assert bool(bad[2]) and bool(bad[4097 - 2])


def test_param_rounded_from_old_master_is_flagged():
    hp, old, pw, new = _adam_emulated(4097, 2, 0.01, "fma")
    assert N.param_bits_ok(new["param"], new["p"])
    assert not N.param_bits_ok(old["p"].to(bf16), new["p"])
    stale = dict(new, param=old["p"].to(bf16))
    assert N.adam_check("", old, stale, N.d(old["g"]), pw, hp, "emu",
                        count_only=True) == 1


def test_multi_tensor_offset_off_by_one_is_flagged():
    hp = N.Hyper(wd=0.01)
    states = [N.adam_state(n, f32, seed=i) for i, n in enumerate(MULTI_SIZES)]
    old = N.multi_concat(states)
    pw = hp.pow_at(2)
    new = N.emu_adam(old, old["g"], pw, hp, "scalar")
    del new["param"]
    g64 = N.d(old["g"])
    assert N.adam_check("", old, new, g64, pw, hp, "emu", scalar_from=0,
                        count_only=True) == 0
    shifted = N.multi_concat(states, shift_state=True)
    assert N.adam_check("", shifted, new, g64, pw, hp, "emu", scalar_from=0,
                        count_only=True) > 0
