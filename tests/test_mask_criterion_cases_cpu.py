"""The float64 references of tests/mask_criterion_cases.py against independent formulations (oracle/mask_criterion_oracle.py run in
float64, and torch.autograd through it), and the properties every case is built for.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from oracle import mask_criterion_oracle as O
from tests import mask_criterion_cases as MC

U32 = MC.U32


def close(a, b, tol=1e-11):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = float(b.abs().max().clamp_min(1e-300))
    assert float((a - b).abs().max()) <= tol * max(scale, 1.0), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ coordinates
def _coords_of(c):
    return [(c["rand_over"], c["w"], c["h"]), (c["rand_over"], c["W"], c["H"]), (c["rand_extra"], c["w"], c["h"]), (c["rand_extra"], c["W"], c["H"])]


@pytest.mark.parametrize("name", [n for n in MC.SET_CASES if not MC.SET_CASES[n][10]])
def test_dyadic_coordinates_have_an_exact_fp32_source_index(name):
    c = MC.set_case(name)
    assert c["g"] + MC.bits(max(c["H"], c["W"])) <= 24
    for co, sx, sy in _coords_of(c):
        for axis, size in ((0, sx), (1, sy)):
            v = co[..., axis]
            assert bool((MC.index32(v, size).double() == MC.index64(v, size)).all()), (name, size)
    assert bool((c["rand_extra"][:, 0] == 0).all()) and bool((c["rand_extra"][:, 1] == 1).all())        # c = 0 and c = 1 are sampled


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("hw", MC.PS_PLANES)
def test_point_sample_cases_are_exact_in_fp32_and_match_grid_sample(hw, u8):
    H, W = hw
    for P in MC.PS_POINTS:
        c = MC.point_sample_case(H, W, P, u8)
        for axis, size in ((0, W), (1, H)):
            v = c["coords"][..., axis]
            assert bool((MC.index32(v, size).double() == MC.index64(v, size)).all())
        si, ci = [5, 0, 2, 2, 1], [4, 1, 1, 0, 3]
        ref, mag = MC.point_sample_ref(c, si, ci)
        want = O.point_sample(c["src"][si][:, None].double(), c["coords"][ci].double())[:, 0]
        close(ref, want)
        assert bool((mag >= ref.abs() - 1e-12).all())
        if P >= 2:      # c = 0 and c = 1: one tap in bounds with weight 1/4
            close(ref[:, 0], c["src"][si][:, 0, 0].double() / 4)
            close(ref[:, 1], c["src"][si][:, -1, -1].double() / 4)


def test_pixel_centres_of_the_power_of_two_plane_are_exact():
    """fp32 grid_sample reproduces a 64 x 32 plane bit for bit at its pixel centres, and does not on 40 x 48: the exact test needs the former."""
    for (H, W), exact in (((64, 32), True), ((40, 48), False)):
        pc = MC.pixel_centres(H, W)
        plane = torch.randn(H, W, generator=MC.gen(1)) * 3
        i32x, i32y = MC.index32(pc[:, 0], W), MC.index32(pc[:, 1], H)
        on_centre = bool((i32x == torch.floor(i32x)).all() and (i32y == torch.floor(i32y)).all())
        got = O.point_sample(plane[None, None], pc[None])[0, 0]
        assert on_centre == exact
        assert torch.equal(got, plane.reshape(-1)) == exact
    ref, _ = MC.sample64(plane := torch.randn(64, 32, generator=MC.gen(2)), MC.pixel_centres(64, 32))
    assert torch.equal(ref, plane.double().reshape(-1))


def test_free_point_sample_case_magnitude_carries_the_coordinate_term():
    c = MC.point_sample_case(40, 48, 257, False, free=True)
    ref, mag = MC.point_sample_ref(c, [0, 1], [0, 1])
    _, mag0 = MC.point_sample_ref(dict(c, free=False), [0, 1], [0, 1])
    close(ref, O.point_sample(c["src"][:2][:, None].double(), c["coords"][:2].double())[:, 0])
    assert bool((mag[:, 5:] > mag0[:, 5:]).all())
    # the fp32 run of the same formula stays within a few roundings of that magnitude
    got = O.point_sample(c["src"][:2][:, None], c["coords"][:2])[:, 0].double()
    assert float(((got - ref).abs() / mag).max()) <= 8 * U32


# ------------------------------------------------------------------------------------------------ match cost
@pytest.mark.parametrize("cls_sigmoid", [False, True])
@pytest.mark.parametrize("case", MC.MATCH_CASES, ids=MC.match_id)
def test_match_cost_reference_vs_oracle(case, cls_sigmoid):
    """matcher_cost takes planes and samples them; on 1 x P planes sampled at their pixel centres the samples are the plane values."""
    c = MC.match_case(case)
    ref, mag = MC.match_cost_ref(c, cls_sigmoid)
    B, Q, P = c["B"], c["Q"], c["P"]
    off = c["offsets"].tolist()
    assert ref.shape == (B, Q, c["Tmax"])
    centres = torch.stack([(torch.arange(P, dtype=torch.float64) + 0.5) / P, torch.full((P,), 0.5, dtype=torch.float64)], 1)[None]
    w_class, w_mask, w_dice = MC.MATCH_W
    for b in range(B):
        T = off[b + 1] - off[b]
        assert bool((ref[b, :, T:] == 0).all()) and bool((mag[b, :, T:] == 0).all())
        if T == 0:
            continue
        x, t = c["pred"][b * Q:(b + 1) * Q].double(), c["tgt"][off[b]:off[b + 1]].double()
        lab = c["labels"][off[b]:off[b + 1]]
        # the oracle's formulation (two BCE sums against ones and zeros) in float64 ...
        pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
        neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
        lg = c["logits"][b].double()
        prob = lg.sigmoid() if cls_sigmoid else lg.softmax(-1)
        s = x.sigmoid()
        want = (w_mask * (pos @ t.T + neg @ (1 - t).T) / P - w_class * prob[:, lab.long()]
                + w_dice * (1 - (2 * s @ t.T + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)))
        close(ref[b, :, :T], want, 1e-11)
        # ... and the oracle itself, which casts the samples to fp32: 1 x P planes sampled at their pixel centres give the plane values
        orc = O.matcher_cost(lg, x.reshape(Q, 1, P), lab, t.reshape(T, 1, P), centres, w_class, w_mask, w_dice, cls_sigmoid)
        close(ref[b, :, :T], orc, 2e-6)
    assert bool((mag >= ref.abs() - 1e-12).all())


def test_match_cases_reach_what_they_claim():
    qs, ps, ks, cs = (set(c[i] for c in MC.MATCH_CASES) for i in (0, 2, 3, 1))
    assert qs == {1, 16, 17, 37} and ps == {1, 63, 64, 65, 777} and ks == {1, 64, 150}
    assert cs == {(0, 21, 40), (3, 5), (64,), (65,)}
    for counts in cs:       # every count set meets every P
        assert {c[2] for c in MC.MATCH_CASES if c[1] == counts} == ps
    # slices of 777 points with 16 splits: 64 points each, 13 slices used, the last holds 9
    per = (-(-777 // MC.mmc_splits(1, 16)) + 63) // 64 * 64
    assert MC.mmc_splits(1, 16) == 16 and per == 64 and 777 - 12 * per == 9


# ------------------------------------------------------------------------------------------------ set loss
def _indices(c):
    off = c["offsets"].tolist()
    return [(c["pred_idx"][off[b]:off[b + 1]].long(), c["tgt_idx"][off[b]:off[b + 1]].long()) for b in range(c["B"])]


def _oracle_losses(c, pred, logits):
    B, Q, K, h, w = c["B"], c["Q"], c["K"], c["h"], c["w"]
    off = c["offsets"].tolist()
    idx = _indices(c)
    tgt = [c["tgt_masks"][off[b]:off[b + 1]].double().reshape(-1, c["H"], c["W"]) for b in range(B)]
    ratio = (c["k_imp"] + 0.5) / c["num_points"]
    lm, ld, coords = O.mask_losses(pred.reshape(B, Q, h, w), tgt, idx, c["num_masks"], c["num_points"], c["rand_over"].double(),
                                   c["rand_extra"].double() if c["n_extra"] else None, ratio)
    target = MC.target_classes(B, Q, K, c["labels"], off, c["pred_idx"], c["tgt_idx"])
    wts = torch.ones(K + 1, dtype=torch.float64)
    wts[-1] = c["eos"]
    ce = F.cross_entropy(logits.reshape(B * Q, K + 1), target.reshape(-1), wts)
    return ce, lm, ld, coords


@pytest.mark.parametrize("gk", list(MC.GRADS))
@pytest.mark.parametrize("name", list(MC.SET_CASES))
def test_set_loss_reference_vs_oracle_and_autograd(name, gk):
    c = MC.set_case(name)
    r = MC.set_ref(name, gk)
    pred = c["pred_masks"].double().clone().requires_grad_(True)
    logits = c["logits"].double().clone().requires_grad_(True)
    ce, lm, ld, _ = _oracle_losses(c, pred, logits)
    w_ce, w_mask, w_dice = c["weights"]
    want = torch.stack([w_ce * ce, w_mask * lm, w_dice * ld])
    close(r["out3"], want.detach(), 1e-10)
    # the oracle's own label_loss (it casts to fp32) agrees to fp32 accuracy
    ll = O.label_loss(c["logits"], [c["labels"][a:b].long() for a, b in zip(c["offsets"][:-1].tolist(), c["offsets"][1:].tolist())],
                      [(i.tolist(), j.tolist()) for i, j in _indices(c)], c["K"], c["eos"])
    assert abs(float(ll) * w_ce - float(r["out3"][0])) <= 2e-5 * float(r["out3"][0])
    g = torch.tensor(MC.GRADS[gk], dtype=torch.float64)
    (want * g).sum().backward()
    close(r["dmasks"], pred.grad, 1e-10)
    close(r["dlogits"], logits.grad.reshape(r["dlogits"].shape), 1e-10)
    assert bool((r["dmasks_mag"] >= r["dmasks"].abs() * (1 - 1e-12)).all()) and bool((r["out3_mag"] >= r["out3"].abs() * (1 - 1e-12)).all())
    rows = MC.matched_rows(c)
    assert int(rows.sum()) == c["sum_T"] and not bool(r["dmasks"][~rows].any())
    assert all(len(s) == c["k_imp"] for s in r["sel"])


@pytest.mark.parametrize("name", list(MC.SET_CASES))
def test_selection_margin(name):
    """The gap between the k_imp-th and the (k_imp + 1)-th smallest |x| is at least 16 x the fp32 sampling error bound (magnitude x 2^-24,
    with the coordinate term in the free case): kernel and reference select the same set."""
    c = MC.set_case(name)
    r = MC.set_ref(name)
    assert 0 < c["k_imp"] < c["n_over"] and len(r["gaps"]) == c["sum_T"]
    for gap, mag in r["gaps"]:
        assert gap >= 16 * mag * U32, (name, gap, 16 * mag * U32)


def test_set_cases_reach_what_they_claim():
    cs = {n: MC.set_case(n) for n in MC.SET_CASES}
    assert MC.bands(40, 48) == (40, 1, 40)
    assert MC.bands(130, 127) == (129, 2, 1)
    assert MC.bands(200, 200) == (81, 3, 38)
    assert MC.bands(3, 16384) == (1, 3, 1) and 1 * 16384 * 4 == 64 * 1024
    assert MC.bands(2, 16385) is None
    assert MC.bands(5, 6) == (5, 1, 5)
    for n, c in cs.items():
        assert (c["H"], c["W"]) == (4 * c["h"], 4 * c["w"])
        assert c["num_masks"] != c["sum_T"] and len(set(c["weights"])) == 3
        off = c["offsets"].tolist()
        for b in range(c["B"]):
            pi = c["pred_idx"][off[b]:off[b + 1]].tolist()
            assert len(set(pi)) == len(pi) and sorted(c["tgt_idx"][off[b]:off[b + 1]].tolist()) == list(range(len(pi)))
    assert cs["one-pair"]["sum_T"] == 1 and cs["one-pair"]["B"] * cs["one-pair"]["Q"] == 5 and cs["one-pair"]["K"] + 1 == 65
    t = cs["three-images"]
    assert t["counts"] == (5, 0, 4) and t["sum_T"] == 9 and t["u8"] and (t["B"] * t["Q"]) % 4 != 0
    assert t["pred_idx"][:5].tolist() != sorted(t["pred_idx"][:5].tolist()) and t["tgt_idx"][:5].tolist() != list(range(5))
    assert cs["two-bands"]["B"] * cs["two-bands"]["Q"] == 7
    m = cs["many-targets"]
    assert max(m["counts"]) > 64 and m["K"] + 1 == 65 and float(m["logits"][0, 3].max()) > 55
    # row-bands: the two tap rows of a point never share a band (band_rows = 1), and points exist whose both rows are inside the plane
    rb = cs["row-bands"]
    iy = MC.index64(rb["rand_over"][..., 1], 3)
    assert bool(((iy >= 0) & (iy < 2)).any())
    # two-bands: points whose taps straddle rows 128 | 129
    tb = cs["two-bands"]
    y0 = torch.floor(MC.index64(torch.cat([tb["rand_over"], tb["rand_extra"]], 1)[..., 1], 130))
    assert bool((y0 == 128).any())
    y0 = torch.floor(MC.index64(torch.cat([cs["three-bands"]["rand_over"], cs["three-bands"]["rand_extra"]], 1)[..., 1], 200))
    assert bool((y0 == 80).any()) and bool((y0 == 161).any())


# ------------------------------------------------------------------------------------------------ the selection run
@pytest.mark.parametrize("k", MC.SEL_K_IMP)
@pytest.mark.parametrize("n_over", MC.SEL_N_OVER)
def test_selection_cases(n_over, k):
    c = MC.selection_case(n_over, k)
    r = MC.selection_ref(n_over, k)
    k_imp = c["k_imp"]
    assert c["chunk"] == (1 if n_over <= 1024 else 2) and c["n_over"] >= c["num_points"] - c["n_extra"]
    assert (k_imp == 0) == (c["n_extra"] == c["num_points"])
    # candidates sit at distinct pixel centres and x is the plane value: multiples of 1/8, exact in fp32
    for n in range(2):
        row = int(c["pred_idx"][n])
        plane = c["pred_masks"][row].reshape(c["h"], c["w"])
        x, _ = MC.sample64(plane, c["rand_over"][n])
        pix, wt = MC.main_tap(c["h"], c["w"], torch.cat([c["rand_over"][n], c["rand_extra"][n]]))
        assert bool((wt == 1).all()) and len(set(pix.tolist())) == pix.numel()
        assert torch.equal(x, plane.reshape(-1)[pix[:n_over]].double()) and bool((x * 8 == torch.round(x * 8)).all())
        ties = c["ties"][n]
        assert ties.numel() == MC.SEL_TIES and bool((x[ties].abs() == MC.SEL_TIE_ABS).all()) and int((x.abs() == MC.SEL_TIE_ABS).sum()) == MC.SEL_TIES
        assert bool((x[ties] > 0).any()) and bool((x[ties] < 0).any())
        sel = r["sel"][n]
        assert sel.numel() == k_imp
        if 0 < k_imp < n_over:
            assert int((x.abs() < MC.SEL_TIE_ABS).sum()) == c["n_below"] == k_imp - c["need"]
            chosen = [i for i in ties.tolist() if i in set(sel.tolist())]
            assert chosen == ties.tolist()[:c["need"]] and c["need"] < MC.SEL_TIES            # the first `need` ties in index order, not all
            assert c["need"] == (MC.SEL_NEED if k_imp >= MC.SEL_NEED else k_imp)
            # the ties sit on different targets: taking another tie instead changes the loss
            t, _ = MC.sample64(c["tgt_masks"][int(c["tgt_idx"][n])].reshape(c["H"], c["W"]), c["rand_over"][n][ties])
            assert bool((t == 0).any()) and bool((t == 1).any())
            if c["chunk"] == 2:
                tl = set(ties.tolist())
                assert any(i % 2 == 0 and i + 1 in tl for i in tl), "two ties inside one thread's chunk"
                assert any(i % 2 == 1 and i + 1 in tl for i in tl), "two ties across a chunk boundary"
        # the oracle selects a set with the same multiset of |x| (torch.topk promises no order among equals)
        if k_imp > 0:
            idx = torch.topk(-x.abs(), k_imp).indices
            assert torch.equal(torch.sort(x.abs()[idx]).values, torch.sort(x.abs()[sel]).values)
    # no selected point has a zero gradient, so the selected set can be read off dmasks
    exp = MC.expected_pixels(c, r)
    assert torch.equal(r["dmasks"] != 0, exp)
    assert int(exp.sum()) == 2 * (k_imp + c["n_extra"])
