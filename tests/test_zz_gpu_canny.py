"""GPU: canny (kornia_amd/filters/canny.py) against the reference's outputs (tests/golden/canny.npz).  The front half runs on
km_filter2d_sep_fwd + km_spatial_gradient_fwd, the back half on km_canny_nms_fwd + km_canny_hysteresis_sweep (fp32 without
autograd; differentiable calls keep the tensor expressions).  Also run through the host build of the kernels
(tests/test_emulated_kernels.py)."""
import pytest
import torch

from _util import golden as _golden_np

pytestmark = pytest.mark.gpu


def golden(name):
    return {k: torch.from_numpy(v) for k, v in _golden_np(name).items()}


def _agree(a, b):
    """fraction of pixels on which two edge maps differ (a threshold crossing may flip on a 1-ulp magnitude difference)"""
    return (a != b).float().mean().item()


def test_canny_vs_reference():
    import kornia_amd as K

    d = golden("canny")
    x = d["x"].cuda()
    mag, edges = K.filters.canny(x)
    assert mag.shape == (2, 1, 48, 64) and edges.shape == (2, 1, 48, 64)
    assert _agree(mag.cpu() > 0, d["mag"] > 0) < 2e-3 and _agree(edges.cpu(), d["edges"]) < 2e-3
    keep = (mag.cpu() > 0) & (d["mag"] > 0)
    assert torch.allclose(mag.cpu()[keep], d["mag"][keep], atol=1e-5, rtol=0)
    mag, edges = K.filters.Canny(hysteresis=False)(x)
    assert _agree(edges.cpu(), d["edges_nohyst"]) < 2e-3 and set(edges.unique().tolist()) <= {0.0, 0.5, 1.0}
    mag, edges = K.filters.canny(x[:, :1], 0.05, 0.3, (3, 3), (0.8, 0.8))
    assert _agree(edges.cpu(), d["edges_gray_k3"]) < 2e-3
    keep = (mag.cpu() > 0) & (d["mag_gray_k3"] > 0)
    assert torch.allclose(mag.cpu()[keep], d["mag_gray_k3"][keep], atol=1e-5, rtol=0)
    assert d["edges"].sum() > 50  # the fixture has edges to find


def test_canny_argument_checks():
    import kornia_amd as K
    from kornia_amd.core.exceptions import BaseError

    x = torch.rand(1, 1, 8, 8).cuda()
    with pytest.raises(BaseError, match="Invalid input thresholds"):
        K.filters.canny(x, 0.3, 0.2)
    with pytest.raises(BaseError, match="Invalid low threshold"):
        K.filters.canny(x, 0.0, 0.2)
    with pytest.raises(BaseError, match="Invalid high threshold"):
        K.filters.Canny(0.1, 1.0)
    with pytest.raises(BaseError):
        K.filters.canny(x[0])
    assert repr(K.filters.Canny())


def test_canny_known_answer_cross():
    """The 5x5 cross of the reference's tests/filters/test_canny.py:85-137 (magnitude and edges, atol 1e-4), its cardinality and
    non-contiguous-input cases (:43-50, 77-83)."""
    import kornia_amd as K

    cross = torch.zeros(1, 1, 5, 5)
    cross[0, 0, 1:4, 2] = 1.0
    cross[0, 0, 2, 1:4] = 1.0
    ring = torch.tensor([[1.2458, 0.9672, 1.2458], [0.9672, 0.0, 0.9672], [1.2458, 0.9672, 1.2458]])
    want_mag, want_edges = torch.zeros(1, 1, 5, 5), torch.zeros(1, 1, 5, 5)
    want_mag[0, 0, 1:4, 1:4] = ring
    want_edges[0, 0, 1:4, 1:4] = (ring > 0).float()
    mag, edges = K.filters.canny(cross.cuda())
    assert torch.allclose(mag.cpu(), want_mag, atol=1e-4, rtol=1e-4) and torch.allclose(edges.cpu(), want_edges, atol=1e-4, rtol=1e-4)
    for batch in (1, 2):
        m, e = K.filters.canny(torch.rand(batch, 3, 4, 4).cuda())
        assert m.shape == (batch, 1, 4, 4) and e.shape == (batch, 1, 4, 4)
    nc = torch.rand(2, 3, 5, 5).cuda().expand(2, -1, -1, -1)[..., ::1]
    m, e = K.filters.canny(nc.transpose(2, 3))
    assert m.is_contiguous() and e.shape == (2, 1, 5, 5)


@pytest.mark.parametrize("shape,hyst", [((2, 3, 70, 130), True), ((1, 1, 64, 64), True), ((2, 1, 33, 200), False)])
def test_canny_native_tail_matches_the_tensor_expressions(shape, hyst):
    """km_canny_nms_fwd + km_canny_hysteresis_sweep against the differentiable composition of the same arithmetic (taken when the
    input requires grad): same magnitude where both keep a pixel, edge maps equal up to threshold crossings of 1-ulp differences, and the
    hysteresis fixed point - long weak chains that cross tile borders included - is the same set of pixels."""
    import kornia_amd as K

    g = torch.Generator().manual_seed(7)
    x = torch.rand(*shape, generator=g)
    # smooth structure so that weak edges form chains: a few blurred blobs on top of the noise
    yy, xx = torch.meshgrid(torch.arange(shape[2], dtype=torch.float32), torch.arange(shape[3], dtype=torch.float32), indexing="ij")
    x = 0.15 * x + 0.85 * (torch.sin(xx / 9.0) * torch.cos(yy / 7.0))[None, None] * 0.5 + 0.4
    xd = x.cuda()
    mag_n, edges_n = K.filters.canny(xd, 0.05, 0.4, hysteresis=hyst)
    mag_c, edges_c = K.filters.canny(xd.clone().requires_grad_(), 0.05, 0.4, hysteresis=hyst)
    mag_c, edges_c = mag_c.detach(), edges_c.detach()
    assert mag_n.shape == mag_c.shape and edges_n.shape == edges_c.shape
    assert _agree(mag_n > 0, mag_c > 0) < 2e-3 and _agree(edges_n, edges_c) < 2e-3
    keep = (mag_n > 0) & (mag_c > 0)
    assert torch.allclose(mag_n[keep], mag_c[keep], atol=1e-6, rtol=0)
    assert set(edges_n.unique().tolist()) <= ({0.0, 1.0} if hyst else {0.0, 0.5, 1.0})
    if hyst:
        assert edges_n.sum() > 0


def test_hysteresis_sweeps_follow_a_chain_across_tiles():
    """km_canny_hysteresis_sweep on a hand-made state: a weak serpentine that crosses the 64 x 64 tile grid many times with ONE strong
    seed at its end must be promoted completely (several sweeps: a sweep carries a promotion only as far as tiles that were already
    consistent), an isolated weak segment must be dropped, and the result must equal the reference's pixel-by-pixel loop."""
    from kornia_amd import _native as N

    lib = N.lib()
    H, W = 150, 200
    state = torch.zeros(1, 1, H, W)
    # serpentine: horizontal runs every 6 rows joined at alternating ends
    rows = list(range(3, H - 3, 6))
    for k, r in enumerate(rows):
        state[0, 0, r, 5:W - 5] = 0.5
        if k + 1 < len(rows):
            c = W - 6 if k % 2 == 0 else 5
            state[0, 0, r:rows[k + 1] + 1, c] = 0.5
    state[0, 0, rows[-1], 5 if len(rows) % 2 == 0 else W - 6] = 1.0  # the seed, at the far end of the chain
    state[0, 0, 1, 20:40] = 0.5  # touches nothing strong (two rows above the first run)
    # the reference's loop (kornia/filters/canny.py:156-176) on the host
    ref = state.clone()
    while True:
        strong = ref == 1
        grown = torch.nn.functional.max_pool2d(strong.float(), 3, 1, 1) > 0
        new = torch.where((ref == 0.5) & grown, torch.ones_like(ref), ref)
        if torch.equal(new, ref):
            break
        ref = new
    want = (ref == 1).float()
    assert want.sum() > (W - 10) * len(rows)  # the whole chain

    st = state.cuda().contiguous()
    out = torch.empty_like(st)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    sweeps = 0
    while True:
        N.check(lib.km_canny_hysteresis_sweep(st.data_ptr(), out.data_ptr(), flag.data_ptr(), 1, H, W, N.stream_ptr(st.device)), "sweep")
        sweeps += 1
        if int(flag.item()) == 0:
            break
        flag.zero_()
        assert sweeps < 200
    assert torch.equal(out.cpu(), want)
    assert 2 <= sweeps <= 2 + len(rows) * 4  # more than one sweep (the chain crosses tiles), far fewer than one per pixel of its length


def _neighbour_code(gx, gy):
    """the reference's direction bin of an integer gradient, 0 .. 7 (east, south-east, ... as in the kernel's table)"""
    import math

    return torch.round(torch.atan2(gy.double(), gx.double()) * (4 / math.pi)).long() % 8


def test_nms_equals_the_reference_tail_exactly():
    """km_canny_nms_fwd against the reference's own magnitude / direction / suppression / threshold code on prepared gradient planes
    (tests/golden/canny_nms.npz, tests/make_golden_canny_nms.py): integers in -12 .. 12 over 32, so every product and sum is exact,
    sqrt is correctly rounded on both sides and no direction sits within 2e-3 of a bin border - magnitude and edges must be EQUAL, with
    eps = 0 and eps = 1e-6.  The fixture has plateaus (ties between a pixel and the neighbour it is compared with, which the strict
    `> 0` must suppress), magnitudes exactly on both thresholds (which the strict `>` must not count) and every one of the 8
    directions; (37, 130) leaves a 2-column last tile, a 5-row last block and a part-filled group of 4 rows."""
    from kornia_amd import _native as N

    d = golden("canny_nms")
    p = d["planes"].long()
    B, _, H, W = p.shape
    scale, low, high = int(d["scale"]), float(d["low"]), float(d["high"])
    assert (B, H, W) == (2, 37, 130) and d["eps"].tolist() == [0.0, 1e-6]
    # the fixture still exercises what it is for (conditions on the input)
    gx, gy = p[:, 0], p[:, 1]
    code = _neighbour_code(gx, gy)
    for k in range(8):
        assert (code == k).float().mean().item() >= 0.05, k
    m2 = torch.nn.functional.pad(gx * gx + gy * gy, (1, 1, 1, 1), value=-1)  # squared magnitude in units of 1 / scale^2: equal iff the magnitudes are
    dy = torch.tensor([0, 1, 1, 1, 0, -1, -1, -1])[code]
    dx = torch.tensor([1, 1, 0, -1, -1, -1, 0, 1])[code]
    bb, ii, jj = torch.meshgrid(torch.arange(B), torch.arange(H), torch.arange(W), indexing="ij")
    centre = m2[bb, ii + 1, jj + 1]
    ties = (m2[bb, ii + 1 + dy, jj + 1 + dx] == centre) | (m2[bb, ii + 1 - dy, jj + 1 - dx] == centre)
    assert ties.sum().item() >= 200
    kept0 = d["mag_eps0"][d["mag_eps0"] > 0]
    assert ((kept0 == low) | (kept0 == high)).sum().item() >= 20

    lib = N.lib()
    grads = (p.float() / scale).cuda().contiguous()  # (B,2,H,W)
    for n, eps in enumerate(d["eps"].tolist()):
        mag = torch.full((B, H, W), -1.0, device="cuda")
        edges = torch.full((B, H, W), -1.0, device="cuda")
        N.check(lib.km_canny_nms_fwd(grads.data_ptr(), mag.data_ptr(), edges.data_ptr(), B, H, W, low, high, eps, N.stream_ptr(grads.device)), "nms")
        want_mag, want_edges = d[f"mag_eps{n}"][:, 0], d[f"edges2_eps{n}"][:, 0].float() / 2
        assert torch.equal(mag.cpu(), want_mag), f"eps={eps}: {(mag.cpu() != want_mag).sum().item()} magnitudes differ"
        assert torch.equal(edges.cpu(), want_edges), f"eps={eps}: {(edges.cpu() != want_edges).sum().item()} edge pixels differ"


def _hysteresis_fixed_point(state):
    """the reference's loop (kornia/filters/canny.py:146-159) on the host: (edges after it, the number of passes it took, the last one included)"""
    ref, passes = state.clone(), 0
    while True:
        grown = torch.nn.functional.max_pool2d((ref == 1).float(), 3, 1, 1) > 0
        new = torch.where((ref == 0.5) & grown, torch.ones_like(ref), ref)
        passes += 1
        if torch.equal(new, ref):
            return (ref == 1).float(), passes
        ref = new


def test_hysteresis_sweeps_at_tile_corners_image_borders_and_between_images():
    """km_canny_hysteresis_sweep where an index slip shows and the serpentine above does not go: a diagonal neighbour across a tile
    corner, the last row of one image against the first row of the next (adjacent in memory, in both roles), the end of a row against
    the start of the next, a weak run that crosses the x = 64 tile border with its seed beyond it, the image corner, and isolated weak
    pixels; then a random state (30 % weak, 3 % strong).  Equal to the reference's loop; a sweep does at least what one pass of that
    loop does, so it needs no more sweeps than the loop needs passes."""
    from kornia_amd import _native as N

    lib = N.lib()
    B, H, W = 2, 70, 130
    hand = torch.zeros(B, 1, H, W)
    hand[0, 0, 63, 63], hand[0, 0, 64, 64] = 0.5, 1.0                # diagonal across the corner of four tiles
    hand[0, 0, H - 1, 10:20], hand[1, 0, 0, 10:20] = 0.5, 1.0        # weak "above" strong across two images: not neighbours
    hand[0, 0, H - 1, 30:40], hand[1, 0, 0, 30:40] = 1.0, 0.5        # and the roles exchanged
    hand[0, 0, 5, W - 1], hand[0, 0, 6, 0] = 1.0, 0.5                # the row wrap: not neighbours
    hand[0, 0, 20, 50:81], hand[0, 0, 21, 80] = 0.5, 1.0             # a run across x = 64, seeded below its far end
    hand[1, 0, H - 1, W - 1], hand[1, 0, H - 2, W - 2] = 0.5, 1.0    # the image corner
    for b, i, j in ((0, 40, 100), (1, 30, 64), (1, 63, 0), (0, 0, 0), (1, 64, 63)):
        hand[b, 0, i, j] = 0.5                                       # isolated weak pixels
    g = torch.Generator().manual_seed(11)
    u = torch.rand(B, 1, H, W, generator=g)
    rand = torch.where(u < 0.03, torch.ones_like(u), torch.where(u < 0.33, torch.full_like(u, 0.5), torch.zeros_like(u)))
    for name, state in (("hand", hand), ("random", rand)):
        want, passes = _hysteresis_fixed_point(state)
        if name == "hand":
            assert want[0, 0, 63, 63] == 1 and want[0, 0, 20, 50:81].all() and want[1, 0, H - 1, W - 1] == 1
            assert want[0, 0, H - 1, 10:20].sum() == 0 and want[1, 0, 0, 30:40].sum() == 0 and want[0, 0, 6, 0] == 0
            assert want.sum() == (state == 1).sum() + 1 + 31 + 1  # nothing else is promoted
        else:
            assert want.sum() > (state == 1).sum() + 100 and ((state == 0.5) & (want == 0)).sum() > 100
        st = state.cuda().contiguous()
        out = torch.full_like(st, -1.0)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        sweeps = 0
        while True:
            N.check(lib.km_canny_hysteresis_sweep(st.data_ptr(), out.data_ptr(), flag.data_ptr(), B, H, W, N.stream_ptr(st.device)), "sweep")
            sweeps += 1
            if int(flag.item()) == 0:
                break
            flag.zero_()
            assert sweeps < 200
        assert torch.equal(out.cpu(), want), f"{name}: {(out.cpu() != want).sum().item()} pixels differ"
        assert 2 <= sweeps <= passes, (name, sweeps, passes)
