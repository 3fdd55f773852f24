"""GPU: one training step of the engine with -rnn_type GRU against the CPU oracle with a GRU layer passed in (`lstm_layer=`): nn.GRU as the
reference builds its recurrences (onmt/Models.py:124-129,140-147, onmt/VI_Model1.py:137-152), decoder initial state = the encoder's final
h alone (onmt/Models.py:1167-1174).  Tiny dims of test_gpu_attention_variants.py, ragged sources, dropout 0, fixed eps; tolerances and the
treatment of the two ill-conditioned image-network tensors are tests/test_gpu_step_parity.py's."""
import pytest
import torch

from oracle import vi1_oracle as O
from tests.test_gpu_step_parity import TOL

pytestmark = pytest.mark.gpu

CONFIGS = {"bi64_l1": dict(hid=64, brnn=True, layers=1),          # no padding, both directions in one launch
           "uni40_l2": dict(hid=40, brnn=False, layers=2)}        # computed 64 wide with zero padding; the layer-to-layer hand-off


def _gru_layer(x, mask, lengths, dirs, h0s, c0s):
    """one nn.GRU layer with the oracle's lstm_layer signature: ignores c0s, returns h in place of c"""
    outs, hs = [], []
    for (w_ih, w_hh, b_ih, b_hh, rev), h in zip(dirs, h0s):
        S, H = x.shape[0], w_hh.shape[1]
        gx, o = x @ w_ih.t() + b_ih, [None] * x.shape[0]
        for t in (range(S - 1, -1, -1) if rev else range(S)):
            a = h @ w_hh.t() + b_hh
            r = torch.sigmoid(gx[t][:, :H] + a[:, :H])
            z = torch.sigmoid(gx[t][:, H:2 * H] + a[:, H:2 * H])
            n = torch.tanh(gx[t][:, 2 * H:] + r * a[:, 2 * H:])
            hn = n + z * (h - n)
            m = 1.0 if mask is None else mask[t].unsqueeze(1)
            h, o[t] = m * hn + (1 - m) * h, m * hn
        outs.append(torch.stack(o)); hs.append(h)
    return (torch.cat(outs, 2) if len(outs) > 1 else outs[0]), hs, hs


@pytest.mark.parametrize("name,dtype", [("bi64_l1", "f32"), ("uni40_l2", "f32"), ("bi64_l1", "bf16")])
def test_gru_step_matches_oracle(name, dtype):
    from variational_mmt_amd.engine import Dims, Engine
    k = CONFIGS[name]
    c = O.Cfg(vs=40, vt=50, emb=32, hid=k["hid"], z=16, img=64, layers=k["layers"], brnn=k["brnn"])
    p = {n: (v[:3 * v.shape[0] // 4].clone() if ".rnn." in n else v) for n, v in O.init_params(c, seed=2).items()}     # 3H recurrent entries
    g = torch.Generator().manual_seed(0)
    B, S, T = 3, 7, 6
    lens = torch.tensor([7, 5, 2])
    src = torch.randint(4, c.vs, (S, B), generator=g)
    for b in range(B):
        src[lens[b]:, b] = 1
    tgt = torch.randint(4, c.vt, (T, B), generator=g)
    table, eps = torch.randn(B, c.img, generator=g), torch.randn(B, c.z, generator=g)
    e = Engine(Dims(c.vs, c.vt, c.emb, c.hid, c.z, c.img, c.layers, c.brnn, 0.0, rnn="GRU"), dtype=dtype, device="cuda", seed=1)
    e.load_state_dict(p)
    e.set_image_table(table)
    ws = e.forward(src, lens, tgt, torch.arange(B), training=True, eps=eps)
    e.loss_backward(ws, normalization=B)
    torch.cuda.synchronize()
    r, Lo, gr = O.step_grads(p, c, src, lens, tgt, table, eps, img_semantic="B", lstm_layer=_gru_layer)
    st, tol = e.read_stats(ws), TOL[dtype]
    print(name, dtype, st["nmt"], float(Lo["nll"]), st["td_kl_before"], float(Lo["kl_before"]), st["elbo"], float(Lo["elbo"]))
    assert abs(st["nmt"] - float(Lo["nll"])) <= tol["loss"] * abs(float(Lo["nll"]))
    assert abs(st["td_kl_before"] - float(Lo["kl_before"])) <= tol["kl"] * abs(float(Lo["kl_before"]))
    assert abs(st["elbo"] - float(Lo["elbo"])) <= tol["loss"] * abs(float(Lo["elbo"]))
    assert sorted(e.grads.keys()) == sorted(gr.keys())
    bad = []
    for n in gr:
        got, want = e.grads[n].detach().cpu().double(), gr[n].double()
        assert got.shape == want.shape, n
        scale, err = max(want.abs().max().item(), 1e-12), (got - want).abs().max().item()
        if dtype == "bf16" and ("inf_net_image.location.fc1" in n or "gate_affine_transform" in n):
            if (got - want).norm().item() > 0.15 * want.norm().item():
                bad.append((n, "relL2", (got - want).norm().item() / want.norm().item()))
        elif err > tol["grad"] * scale + 1e-9:
            bad.append((n, err, scale))
    assert not bad, bad
