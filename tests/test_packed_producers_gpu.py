"""-m gpu: producers that write their result as a packed bf16x3 operand (uda_bnbwd_apply_x3, uda_bnbwd_apply_lowrank_x3,
uda_upconv_bwd_x3).  The packed bytes equal, byte for byte, uda_x3_pack of the fp32 result of the unchanged entry on the same inputs;
in dual-write mode the fp32 result is bit-identical too.  Every destination sits between guard bytes / guard rows that stay untouched,
and so does a poisoned fp32 matrix that is NOT handed in when only the packed form is asked for.  Last: the generator's backward
with the packed producers on and off gives bit-identical gradients at a size where all three matrices take the packed path."""
import pytest
import torch

from uda_clr_amd.acts import ACT_NONE, ACT_RELU, Act, BNRec, round4

pytestmark = pytest.mark.gpu

GUARD = 4096              # bytes of 0xA5 on both sides of a packed destination
GUARD_ROWS = 8            # poisoned rows on both sides of an fp32 destination
ROWS = (1, 255, 256, 257, 2 * 5 * 7)       # around the 256 octets of a packing workgroup; N*H*W = 2*5*7


@pytest.fixture(scope="module")
def K():
    from uda_clr_amd.kernels import HipKernels
    return HipKernels("bf16x3")


def _dev():
    return torch.device("cuda:0")


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(_dev())


def _frame(P, C, ld):
    """-> (poisoned [GUARD_ROWS + P + GUARD_ROWS, ld] frame, its [P, C] window)"""
    f = torch.full((P + 2 * GUARD_ROWS, ld), float("nan"), dtype=torch.float32, device=_dev())
    f.view(torch.int32).fill_(0x7FC0A5A5)
    return f, f[GUARD_ROWS:GUARD_ROWS + P, :C]


def _outside_untouched(frame, P, C):
    bits = frame.view(torch.int32)
    return bool((bits[:GUARD_ROWS] == 0x7FC0A5A5).all() and (bits[GUARD_ROWS + P:] == 0x7FC0A5A5).all()
                and (bits[:, C:] == 0x7FC0A5A5).all())


def _packed_buf(K, rows, Cc):
    """-> (0xA5 buffer with GUARD bytes on both sides, its window of uda_x3_packed_bytes(rows, Cc) bytes, bytes of the body)"""
    n = int(K.lib.uda_x3_packed_bytes(rows, Cc))
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=_dev())
    return buf, buf[GUARD:GUARD + n], rows * ((Cc + 15) // 16) * 96


def _guards_untouched(buf, body):
    """the guards and the 64 bytes behind the body that nobody writes"""
    return bool((buf[:GUARD] == 0xA5).all() and (buf[GUARD + body:] == 0xA5).all())


def _pack(K, m):
    """uda_x3_pack of the raw fp32 matrix ``m`` -> (buffer, window, body bytes)"""
    P, Cc = m.shape
    buf, win, body = _packed_buf(K, P, Cc)
    K.x3_pack(K._src(Act(m, 1, 1, P)), P, Cc, m.device, out=win)
    return buf, win, body


# ---------------------------------------------------------------------------------------------- BatchNorm backward, apply pass
def _bn_case(g, P, C, ld, mask, frozen):
    x = _rand(g, P, ld)[:, :C]
    sc, sh = (0.5 + torch.rand(C, generator=g)).to(_dev()), (0.3 * torch.randn(C, generator=g)).to(_dev())
    mean, istd = (0.1 * torch.randn(C, generator=g)).to(_dev()), (0.5 + torch.rand(C, generator=g)).to(_dev())
    mb = None
    if mask:
        mbuf = torch.zeros(P, round4(ld), dtype=torch.uint8)
        mbuf[:, :C] = (torch.rand(P, C, generator=g) > 0.1).to(torch.uint8)
        mb = mbuf.to(_dev())[:, :C]
    rec = BNRec("t", mean, istd, float("inf") if frozen else float(P), False, frozen=frozen)
    y = Act(x, 1, 1, P, sc, sh, ACT_RELU, mb, 1.0 / 0.9 if mask else 1.0, rec)
    if frozen:          # what uda_bnbwd_finalize gives for count = inf
        c1, c2 = torch.zeros(C, device=_dev()), torch.zeros(C, device=_dev())
    else:
        c1, c2 = 0.1 * _rand(g, C), 0.1 * _rand(g, C)
    return y, c1, c2


@pytest.mark.parametrize("C", [16, 24, 40, 256])
@pytest.mark.parametrize("k", [0, 1, 2], ids=["matrix", "lowrank1", "lowrank2"])
def test_bnbwd_apply_packed_equals_pack_of_fp32(K, C, k):
    g = torch.Generator().manual_seed(100 * C + k)
    variants = [(P, C, False, False, False) for P in ROWS]                      # (rows, row stride, addend, mask, frozen)
    variants += [(257, C + 12, True, False, False), (70, C + 12, True, True, False), (255, C, True, False, True), (256, C + 4, False, True, True)]
    for P, ld, with_add, mask, frozen in variants:
        y, c1, c2 = _bn_case(g, P, C, ld, mask, frozen)
        dU = _rand(g, P, ld)[:, :C]
        ad = _rand(g, P, ld)[:, :C] if with_add else None
        if k:
            wide = _rand(g, P, 8)
            lr = {"lowrank": (wide[:, 4:4 + k], _rand(g, k, C) / C ** 0.5)}
            dU = None
        else:
            lr = {}
        tag = "P %d C %d ld %d addend %s mask %s frozen %s" % (P, C, ld, with_add, mask, frozen)
        # the unchanged entry, then the packing pass over its result
        f_ref, o_ref = _frame(P, C, ld)
        K.bnbwd_apply(dU, y, c1, c2, o_ref, ad, **lr)
        _, p_ref, body = _pack(K, o_ref)
        # packed form only: a poisoned fp32 matrix nearby is not handed in and stays as it is
        f_near, _ = _frame(P, C, ld)
        buf, win, _ = _packed_buf(K, P, C)
        K.bnbwd_apply(dU, y, c1, c2, None, ad, out_x3=win, **lr)
        assert torch.equal(win[:body], p_ref[:body]), tag
        assert _guards_untouched(buf, body), tag
        assert bool((f_near.view(torch.int32) == 0x7FC0A5A5).all()), tag
        # both forms in one pass
        f_two, o_two = _frame(P, C, ld)
        buf2, win2, _ = _packed_buf(K, P, C)
        K.bnbwd_apply(dU, y, c1, c2, o_two, ad, out_x3=win2, **lr)
        assert torch.equal(f_two.view(torch.int32), f_ref.view(torch.int32)), tag
        assert _outside_untouched(f_two, P, C), tag
        assert torch.equal(win2[:body], p_ref[:body]) and _guards_untouched(buf2, body), tag
        if not k:       # in place over dU, as the engine's dy1
            f_in, o_in = _frame(P, C, ld)
            o_in.copy_(dU)
            buf3, win3, _ = _packed_buf(K, P, C)
            K.bnbwd_apply(o_in, y, c1, c2, o_in, ad, out_x3=win3)
            assert torch.equal(o_in.contiguous().view(torch.int32), o_ref.contiguous().view(torch.int32)), tag
            assert _outside_untouched(f_in, P, C), tag
            assert torch.equal(win3[:body], p_ref[:body]) and _guards_untouched(buf3, body), tag


def test_packed_only_matrix_is_marked_and_has_no_fp32_side(K):
    m, xs = K.packed_out(70, 24, _dev())
    assert K._x3_only(m) and m._x3 is xs and K._x3_dst(m, xs, 70, 24)[0] is None
    both, xs2 = K.packed_out(70, 24, _dev(), fp32=torch.empty(70, 24, device=_dev()))
    assert not K._x3_only(both) and both._x3 is xs2 and K._x3_dst(both, xs2, 70, 24)[0] == both.data_ptr()


# ---------------------------------------------------------------------------------------------- adjoint of the interpolated taps
UPCONV = [(2, 5, 5, 17, 17, 256), (2, 3, 7, 9, 25, 256), (2, 4, 4, 4, 4, 256),              # C = 256: a wave per pixel
          (2, 5, 5, 17, 17, 32), (2, 3, 7, 9, 25, 48), (2, 4, 4, 4, 4, 32), (1, 3, 3, 9, 9, 4)]    # a thread per (pixel, granule); 9 * 4 columns: ragged


@pytest.mark.parametrize("N, h, w, H, W, C", UPCONV, ids=["%dx%dx%d_to_%dx%d_C%d" % s for s in UPCONV])
def test_upconv_bwd_packed_equals_pack_of_fp32(K, N, h, w, H, W, C):
    g = torch.Generator().manual_seed(7 * C + H)
    assert K.upconv_route("bwd", N, h, w, H, W, C).startswith("bwd wave" if C == 256 else "bwd thread")
    P, Q = N * H * W, N * h * w
    for ldy, ldg in ((C, 9 * C), (C + 8, 9 * C + 12)):
        tag = "ldy %d ldg %d" % (ldy, ldg)
        dy = _rand(g, P, ldy)[:, :C]
        f_ref, g_ref = _frame(Q, 9 * C, ldg)
        K.upconv_bwd(dy, N, H, W, g_ref, h, w)
        _, p_ref, body = _pack(K, g_ref)
        f_near, _ = _frame(Q, 9 * C, ldg)
        buf, win, _ = _packed_buf(K, Q, 9 * C)
        K.upconv_bwd(dy, N, H, W, None, h, w, dg_x3=win)
        assert torch.equal(win[:body], p_ref[:body]) and _guards_untouched(buf, body), tag
        assert bool((f_near.view(torch.int32) == 0x7FC0A5A5).all()), tag
        f_two, g_two = _frame(Q, 9 * C, ldg)
        buf2, win2, _ = _packed_buf(K, Q, 9 * C)
        K.upconv_bwd(dy, N, H, W, g_two, h, w, dg_x3=win2)
        assert torch.equal(f_two.view(torch.int32), f_ref.view(torch.int32)) and _outside_untouched(f_two, Q, 9 * C), tag
        assert torch.equal(win2[:body], p_ref[:body]) and _guards_untouched(buf2, body), tag


# ---------------------------------------------------------------------------------------------- the generator's backward
def test_generator_backward_is_bit_identical_with_packed_producers(K):
    """B = 16 at 256 x 256: P4 = 65536 and P16 = 4096 rows, the smallest batch at which the library routes the readers of dy2, dy1 and
    dG to the bf16x3 kernels (its predicates are asserted, so the comparison is not one path against itself)."""
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    N, S = 16, 256
    H4, H16 = S // 4, S // 16
    assert K.wgrad_route_x3(N, H4, H4, 256, 256, 3) and K.conv_route_x3(N, H4, H4, 256, 256, 3)
    assert K.wgrad_route_x3(N, H4, H4, 48, 256, 3) and K.conv_route_x3(N, H4, H4, 256, 48, 3)
    assert K.wgrad_route_x3(N, H16, H16, 256, 2304, 1) and K.conv_route_x3(N, H16, H16, 2304, 256, 1)
    torch.manual_seed(3)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(_dev())
    model.train()
    from uda_clr_amd.engine import GeneratorEngine
    model._engine = GeneratorEngine(K, model.output_stride, backbone=model.backbone_name)
    x = torch.rand(N, 3, S, S, generator=torch.Generator().manual_seed(4)).to(_dev())
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads = []
    for on in (True, False):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        model._engine._x3_producers = on
        model._engine.rng_offset = 0
        outs = model(x)
        loss = sum((o.float() ** 2).mean() for o in outs if torch.is_tensor(o) and o.requires_grad)
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    model._engine._x3_producers = True
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 100
    bad = [n for n in grads[0] if not torch.equal(grads[0][n].view(torch.int32), grads[1][n].view(torch.int32))]
    assert not bad, bad[:5]


# ---------------------------------------------------------------------------------------------- whole trainer steps
@pytest.mark.parametrize("kind", ["baseline", "proto"])
def test_trainer_step_is_bit_identical_with_packed_producers(tmp_path, kind):
    """One Trainer_baseline / Trainer_prototype_full step at 64 x 64, B = 2 (+ 2), bf16x3 mode, from the same seed with the packed
    producers on and off: the same losses and the same parameters after the step, bit for bit.  (At this size the library routes
    the three matrices' readers to the fp32-row kernels, so both runs also check that the engine then leaves the fp32 path alone;
    the test above compares the two paths where they differ.)"""
    import model_cases
    import step_cases
    from uda_clr_amd.engine import GeneratorEngine
    from uda_clr_amd.kernels import HipKernels
    results = []
    for on in (True, False):
        gen = model_cases.seeded_model(perturb=kind == "baseline").to(_dev())
        gen._engine = GeneratorEngine(HipKernels("bf16x3"), gen.output_stride, backbone=gen.backbone_name)
        gen._engine._x3_producers = on
        step_cases.RecordingDeepLab.adopt(gen)
        tr = step_cases.make_trainer(kind, gen, _dev(), tmp_path / ("on" if on else "off"), 64, 2)
        gen.train()
        if kind == "proto":
            tr.model_dis.train()
            tr.model_dis2.train()
        s, t = step_cases.batches(kind, 2, 64, 1)[0]
        row = step_cases.product_step(tr, kind, s, t)
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in gen.state_dict().items()}
        if kind == "proto":
            state.update({"dis." + k: v.detach().clone() for k, v in tr.model_dis.state_dict().items()})
            state.update({"dis2." + k: v.detach().clone() for k, v in tr.model_dis2.state_dict().items()})
        results.append(({k: float(v) for k, v in row.items()}, state))
    (row_on, st_on), (row_off, st_off) = results
    assert row_on == row_off, (row_on, row_off)
    assert st_on.keys() == st_off.keys()
    bad = [k for k in st_on if not torch.equal(st_on[k], st_off[k])]
    assert not bad, bad[:5]
