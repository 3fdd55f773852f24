"""GPU: the `dot` and `mlp` attention variants (-global_attention, onmt/modules/GlobalAttention.py:70-78,114-127,187-190) through the engine,
the model constructor, the state dict and the decoder.
  * dot: one fp32 training step at the tiny fixture dims against the CPU oracle with decoder.attn.linear_in.weight = I (the `general` score
    with an identity is the dot score); test_gpu_step_parity.py's fp32 tolerances, same quantities and precision.
  * mlp: the gradient of a training step against central differences of its own loss, (L(theta + h delta) - L(theta - h delta)) / 2h against
    <grad L, delta>, L = ELBO / B in fp32, dropout 0, fixed noise.  delta: three fixed N(0, 1) directions over the whole gradient arena and
    the first of them restricted to the attention parameters.  h = H_STEP (a step of 1 % of the parameters' init scale 0.1 per element).
    The bound is measured: the identical check with attn = "general" -- a path pinned to the oracle -- shows what fp32 differencing yields
    at this h; FLOOR is its largest relative error over the four directions and the two configurations, the bound is twice that.
    Measured at h = 1e-3, directions 1-3 whole arena, 4 attention only:
        general  bi64   1.85e-2  1.71e-1  5.72e-2  1.01e-1      uni40  4.96e-3  2.99e-2  1.36e-2  1.27e-3      FLOOR = 1.71e-1
        mlp      bi64   1.88e-2  3.81e-2  6.38e-4  6.45e-4      uni40  1.22e-2  2.81e-2  6.68e-2  3.39e-3      BOUND = 3.42e-1
    (the whole-arena figures do not shrink with h, 3e-4 .. 3e-3: the step's gradient is not the derivative of the reported ELBO along
    every parameter -- the sample is detached and the image term is differentiated as executed, DESIGN section 2 -- so the floor is that
    mismatch, not rounding.)  One direction per attention parameter was tried as well and is NOT part of the test: in a model this small
    dL/dW_q, dL/db_q, dL/dv and dL/dW_c along a random direction are 5e-4 .. 5e-3, at or below what differencing an fp32 ELBO resolves
    (about 3e-4 at this h), for `general`'s linear_in just the same.
  * dot, mlp: make_vi_model_mmt builds the model; state_dict() carries exactly the reference's names and shapes; load_state_dict(strict=True)
    round-trips bit-exactly; the round-tripped model translates three ragged sentences with beam 2 to the end, and the first position's
    attention row matches an fp64 evaluation of the score from the same decoder state (2e-5: test_gpu_step_parity.py's fp32 activations)."""
import types

import pytest
import torch

from oracle import vi1_oracle as O
from tests.golden_util import load
from tests.test_gpu_onmt_surface import _opt, _Vocab

pytestmark = pytest.mark.gpu

TOL = dict(loss=2e-5, kl=2e-5, grad=2e-4, act=2e-5)          # test_gpu_step_parity.py, f32
ATTN_NAMES = {"dot": {"linear_out.weight": (1, 2)},
              "mlp": {"linear_out.weight": (1, 2), "linear_out.bias": (1,), "linear_query.weight": (1, 1), "linear_query.bias": (1,),
                      "linear_context.weight": (1, 1), "v.weight": (0, 1)}}          # shape in units of H (0: the literal 1)
CONFIGS = {"bi64": dict(hid=64, brnn=True),          # H = 64: no padding
           "uni40": dict(hid=40, brnn=False)}        # uni-directional, H % 32 != 0: computed 64 wide with zero padding (Dims.hp)
H_STEP = 1e-3
FLOOR = 1.71e-1
BOUND = 2 * FLOOR


def _central_differences(attn, cfg, h):
    """[(numeric, analytic, relative error)] for the four directions"""
    from variational_mmt_amd.engine import Dims, Engine
    c = CONFIGS[cfg]
    e = Engine(Dims(40, 50, 32, c["hid"], 16, 64, 1, c["brnn"], 0.0, attn=attn), dtype="f32", device="cuda", seed=3, param_init=0.1)
    g = torch.Generator().manual_seed(0)
    B, S, T = 3, 7, 6
    lens = torch.tensor([7, 5, 2])
    src = torch.randint(4, 40, (S, B), generator=g)
    for b in range(B):
        src[lens[b]:, b] = 1
    tgt = torch.randint(4, 50, (T, B), generator=g)
    e.set_image_table(torch.randn(B, 64, generator=g))
    eps = torch.randn(B, 16, generator=g)

    def loss():
        e.shadows_dirty = True
        ws = e.forward(src, lens, tgt, torch.arange(B), training=True, eps=eps)
        e.loss_backward(ws, normalization=B)
        torch.cuda.synchronize()
        return e.read_stats(ws)["elbo"] / B
    loss()
    grad, theta, n = e.flat_g.double().clone(), e.flat_p.clone(), e.flat_g.numel()
    dirs = [torch.randn(n, generator=torch.Generator().manual_seed(10 + i)).cuda() for i in range(3)]
    mask = torch.zeros(n, device="cuda")
    for k, (o, shp) in e.offsets.items():
        if k.startswith("decoder.attn.") and k in e.grads:
            mask[o:o + e.grads[k].numel()] = 1
    dirs.append(dirs[0] * mask)
    out = []
    for dlt in dirs:
        ls = []
        for sign in (1.0, -1.0):
            e.flat_p.copy_(theta)
            e.flat_p[:n] += sign * h * dlt
            ls.append(loss())
        e.flat_p.copy_(theta)
        num, ana = (ls[0] - ls[1]) / (2 * h), float((grad * dlt.double()).sum())
        out.append((num, ana, abs(num - ana) / abs(ana)))
    return out


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_mlp_gradients_match_central_differences(cfg):
    errs = [r[2] for r in _central_differences("mlp", cfg, H_STEP)]
    assert len(errs) == 4
    assert max(errs) <= BOUND, errs


@pytest.mark.parametrize("name", ["tiny_uni_l2", "tiny_bi_l1"])
def test_dot_step_matches_oracle_with_identity_linear_in(name):
    from variational_mmt_amd.engine import Dims, Engine
    c, p, bt, z, (B, S, T) = load(name)
    p = dict(p)
    p["decoder.attn.linear_in.weight"] = torch.eye(c.hid)
    e = Engine(Dims(c.vs, c.vt, c.emb, c.hid, c.z, c.img, c.layers, c.brnn, 0.0, attn="dot"), dtype="f32", device="cuda", seed=1)
    e.load_state_dict({k: v for k, v in p.items() if k != "decoder.attn.linear_in.weight"})
    e.set_image_table(bt["table"])
    ws = e.forward(bt["src"], bt["src_len"], bt["tgt"], bt["indices"], training=True, eps=bt["eps"])
    e.loss_backward(ws, normalization=B)
    torch.cuda.synchronize()
    img = bt["table"][bt["indices"]]
    r, Lo, g = O.step_grads(p, c, bt["src"], bt["src_len"], bt["tgt"], img, bt["eps"], img_semantic="B")
    st = e.read_stats(ws)
    assert abs(st["nmt"] - float(Lo["nll"])) <= TOL["loss"] * abs(float(Lo["nll"]))
    assert abs(st["td_kl_before"] - float(Lo["kl_before"])) <= TOL["kl"] * abs(float(Lo["kl_before"]))
    assert abs(st["elbo"] - float(Lo["elbo"])) <= TOL["loss"] * abs(float(Lo["elbo"]))
    assert sorted(e.grads.keys()) == sorted(k for k in g if k != "decoder.attn.linear_in.weight")
    for k in e.grads:
        got, want = e.grads[k].detach().cpu().double(), g[k].double()
        assert (got - want).abs().max().item() <= TOL["grad"] * max(want.abs().max().item(), 1e-12) + 1e-9, k


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("attn", ["dot", "mlp"])
def test_surface_checkpoint_round_trip_and_translation(attn, cfg, tmp_path):
    import variational_mmt_amd
    from variational_mmt_amd.decode import _encode
    from variational_mmt_amd.onmt.translate import GNMTGlobalScorer, TranslatorMultimodalVI
    onmt = variational_mmt_amd.install_as_onmt()
    H, brnn = CONFIGS[cfg]["hid"], CONFIGS[cfg]["brnn"]
    c = O.Cfg(vs=43, vt=47, emb=16, hid=H, z=8, img=2048, layers=1, brnn=brnn)
    fields = {"src": types.SimpleNamespace(vocab=_Vocab(c.vs, False)), "tgt": types.SimpleNamespace(vocab=_Vocab(c.vt, True))}
    opt = _opt(c, tmp_path)
    opt.global_attention, opt.seed = attn, 5
    m = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    got = {k[len("decoder.attn."):]: tuple(v.shape) for k, v in sd.items() if k.startswith("decoder.attn.")}
    assert got == {k: tuple(H * u if u else 1 for u in shp) for k, shp in ATTN_NAMES[attn].items()}
    opt.seed = 6
    ck = {"model": {k: v.cpu() for k, v in sd.items() if not k.startswith("generator.")},
          "generator": {k[len("generator."):]: v.cpu() for k, v in sd.items() if k.startswith("generator.")}}
    m2 = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, ck)          # strict load of the reference's names
    sd2 = m2.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    m2.eval()
    # three ragged sentences, beam 2, to the end
    g = torch.Generator().manual_seed(1)
    S, B, K, max_len = 9, 3, 2, 12
    lens = torch.tensor([9, 6, 2])
    src = torch.randint(2, c.vs, (S, B), generator=g)
    for b in range(B):
        src[lens[b]:, b] = 1
    tr = TranslatorMultimodalVI(m2, fields, beam_size=K, n_best=1, max_length=max_len, global_scorer=GNMTGlobalScorer(0.0, 0.0))
    ret = tr.translate_batch(types.SimpleNamespace(src=(src, lens)))
    assert len(ret["predictions"]) == B and all(1 <= len(p[0]) <= max_len for p in ret["predictions"])
    # the first position's attention row against fp64 math from the same state: r_0 and the memory of the evaluation forward
    e = m2.engine
    ws = _encode(e, src.to(e.dev), lens, 2)
    torch.cuda.synchronize()
    r0 = ws.cat.view()[:B, e.d.hp:e.d.hp + H].double().cpu()                                  # [B][H]
    hs = ws.enc_out[-1].view()[:, :H].double().cpu().view(S, B, H)
    P = {k: v.double().cpu() for k, v in sd.items() if k.startswith("decoder.attn.")}
    if attn == "dot":
        sc = torch.einsum("bh,sbh->bs", r0, hs)
    else:
        wq = r0 @ P["decoder.attn.linear_query.weight"].t() + P["decoder.attn.linear_query.bias"]
        uh = hs @ P["decoder.attn.linear_context.weight"].t()
        sc = torch.tanh(wq[None] + uh).permute(1, 0, 2) @ P["decoder.attn.v.weight"][0]
    pr = torch.softmax(sc.masked_fill(torch.arange(S).view(1, S) >= lens.view(B, 1), float("-inf")), dim=1)
    for b in range(B):
        a = ret["attention"][b][0]
        assert tuple(a.shape) == (len(ret["predictions"][b][0]), int(lens[b]))
        assert (a[0].double() - pr[b, :int(lens[b])]).abs().max().item() <= TOL["act"]
