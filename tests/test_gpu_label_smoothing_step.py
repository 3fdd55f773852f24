"""GPU: one training step of the engine with label_smoothing = 0.1 against the CPU oracle, whose NLL term is replaced by
torch.nn.KLDivLoss(reduction="sum") against the smoothed target distribution of onmt/Loss.py:156-166 / onmt/VILoss.py:232-240.  Ragged targets
(pads occur), dropout 0, fixed eps.  Statistics as the reference executes them: `nmt` = the smoothed sum, `elbo` = minus the summed target
log-likelihood alone (VILoss.py:479-480).  Tolerances and the treatment of the two ill-conditioned image-network tensors are
tests/test_gpu_step_parity.py's."""
import pytest
import torch

from oracle import vi1_oracle as O
from tests.test_gpu_step_parity import TOL

pytestmark = pytest.mark.gpu
PAD, EPS = 1, 0.1
# tiny f32 (test_gpu_gru_step.py's dims): the G^T path; bf16 with hid 256: the fused sweep, at a token count the compacted generator serves
CONFIGS = {"tiny_f32": (dict(vs=40, vt=50, emb=32, hid=64, z=16, img=64, layers=1, brnn=True), (3, 7, 6), "f32"),
           "fused_bf16": (dict(vs=300, vt=400, emb=64, hid=256, z=32, layers=1, brnn=True), (128, 12, 13), "bf16")}


def smoothed_kld(p, c, r, tgt, eps):
    """KLDivLoss(sum) of the oracle's generator output against the smoothed targets (Loss.py:156-166, VILoss.py:232-243)"""
    y = tgt[1:].reshape(-1)
    logp = torch.log_softmax(r["out"].reshape(y.numel(), c.hid) @ p["generator.0.weight"].t() + p["generator.0.bias"], 1)
    q = torch.full((1, c.vt), eps / (c.vt - 2), dtype=logp.dtype)
    q[0, PAD] = 0
    q = q.repeat(y.numel(), 1).scatter_(1, y.unsqueeze(1), 1.0 - eps)
    q[y == PAD] = 0
    return torch.nn.KLDivLoss(reduction="sum")(logp, q)


def _engine_and_batch(name):
    from variational_mmt_amd.engine import Dims, Engine
    kw, (B, S, T), dtype = CONFIGS[name]
    c = O.Cfg(**kw)
    p = O.init_params(c, seed=2)
    bt = O.synth_batch(c, B, S, T, n_img=max(B, 4), seed=5, fixed_len=False)
    e = Engine(Dims(c.vs, c.vt, c.emb, c.hid, c.z, c.img, c.layers, c.brnn, 0.0), dtype=dtype, device="cuda", seed=1)
    e.load_state_dict(p)
    e.set_image_table(bt["table"])
    return c, p, bt, e, B, dtype


@pytest.mark.parametrize("name", list(CONFIGS))
def test_smoothed_step_matches_oracle(name):
    c, p, bt, e, B, dtype = _engine_and_batch(name)
    ws = e.forward(bt["src"], bt["src_len"], bt["tgt"], bt["indices"], training=True, eps=bt["eps"])
    e.loss_backward(ws, normalization=B, label_smoothing=EPS)
    torch.cuda.synchronize()
    assert ws.gen_fused == (name == "fused_bf16")
    # the oracle, its NLL term replaced by the KL divergence against the smoothed targets
    pp = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    img = bt["table"][bt["indices"]]
    r = O.forward(pp, c, bt["src"], bt["src_len"], bt["tgt"], img, bt["eps"], True)
    Lo = O.loss(pp, c, r, bt["tgt"], img)
    kld = smoothed_kld(pp, c, r, bt["tgt"], EPS)
    ((Lo["loss"] - Lo["nll"] + kld) / B).backward()
    st, tol, kld, nll = e.read_stats(ws), TOL[dtype], float(kld.detach()), float(Lo["nll"].detach())
    print(name, "nmt", st["nmt"], kld, "elbo", st["elbo"], nll, "tokens per launch", ws.gen_Mc, "of", ws.M)
    assert abs(st["nmt"] - kld) <= tol["loss"] * abs(kld)
    assert abs(st["elbo"] - nll) <= tol["loss"] * abs(nll)
    assert st["n_words"] == Lo["n_words"]
    bad = []
    for n, v in ((n, v) for n, v in pp.items() if v.grad is not None):
        got, want = e.grads[n].detach().cpu().double(), v.grad.double()
        scale, err = max(want.abs().max().item(), 1e-12), (got - want).abs().max().item()
        if dtype == "bf16" and ("inf_net_image.location.fc1" in n or "gate_affine_transform" in n):
            if (got - want).norm().item() > 0.15 * want.norm().item():
                bad.append((n, "relL2", (got - want).norm().item() / want.norm().item()))
        elif err > tol["grad"] * scale + 1e-9:
            bad.append((n, err, scale))
    assert not bad, bad


def test_plans_without_smoothing_have_no_smoothing_entry():
    c, p, bt, e, B, dtype = _engine_and_batch("tiny_f32")
    # kernel entries by name, event entries by the event's name
    names = lambda ws: [en[2] if en[0] is not None else str(en[1])
                        for P in (ws.plan_fwd_train, ws.plan_loss_train, ws.plan_loss_eval, ws.plan_bwd) for en in P]
    ws = e.forward(bt["src"], bt["src_len"], bt["tgt"], bt["indices"], training=True, eps=bt["eps"])
    e.loss_backward(ws, normalization=B)
    plain = names(ws)
    assert not [n for n in plain if n.startswith(("vmmt_ls_", "ls_"))] and ws.ls_buf is None and e.label_smoothing == 0.0
    e.loss_backward(ws, normalization=B, label_smoothing=EPS)          # 0 -> non-0: the plans are rebuilt with the three entries
    assert [n for n in names(ws) if n.startswith("vmmt_ls_")] == ["vmmt_ls_colsum", "vmmt_ls_colsum", "vmmt_ls_rows", "vmmt_ls_dW"]
    e.loss_backward(ws, normalization=B, label_smoothing=0.0)          # and back: exactly the lists of before
    assert names(ws) == plain
    torch.cuda.synchronize()
