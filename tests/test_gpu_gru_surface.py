"""GPU: -rnn_type GRU through the model constructor, the state dict and the decoder.  make_vi_model_mmt builds the model; state_dict() has the
reference's recurrent names with 3H shapes (getattr(nn, "GRU"): onmt/Models.py:124-129, onmt/VI_Model1.py:137-152) and no names beyond the
LSTM model's; load_state_dict(strict=True) round-trips bit-exactly; the round-tripped model translates three ragged sentences with beam 2
to the end; the decoder's first-position state matches an fp64 GRU cell evaluated from the encoder's final h (onmt/Models.py:1167-1174),
the BOS embedding and z (2e-5: test_gpu_step_parity.py's fp32 activations).  GRU with --conditional is refused by name."""
import types

import pytest
import torch

from oracle import vi1_oracle as O
from tests.test_gpu_attention_variants import CONFIGS
from tests.test_gpu_onmt_surface import _opt, _Vocab

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_gru_surface_checkpoint_round_trip_and_translation(cfg, tmp_path):
    import variational_mmt_amd
    from variational_mmt_amd.decode import _encode
    from variational_mmt_amd.onmt.translate import GNMTGlobalScorer, TranslatorMultimodalVI
    onmt = variational_mmt_amd.install_as_onmt()
    H, brnn = CONFIGS[cfg]["hid"], CONFIGS[cfg]["brnn"]
    Hd = H // (2 if brnn else 1)
    c = O.Cfg(vs=43, vt=47, emb=16, hid=H, z=8, img=2048, layers=1, brnn=brnn)
    fields = {"src": types.SimpleNamespace(vocab=_Vocab(c.vs, False)), "tgt": types.SimpleNamespace(vocab=_Vocab(c.vt, True))}
    opt = _opt(c, tmp_path)
    opt.compute_dtype, opt.seed = "f32", 5
    lstm_names = set(onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None).state_dict().keys())
    opt.rnn_type = "GRU"
    m = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert set(sd.keys()) == lstm_names
    want = {"decoder.rnn.weight_ih_l0": (3 * H, c.emb + c.z), "decoder.rnn.weight_hh_l0": (3 * H, H), "decoder.rnn.bias_ih_l0": (3 * H,),
            "decoder.rnn.bias_hh_l0": (3 * H,)}
    for suf in [""] + (["_reverse"] if brnn else []):
        want.update({"encoder.rnn.weight_ih_l0" + suf: (3 * Hd, c.emb), "encoder.rnn.weight_hh_l0" + suf: (3 * Hd, Hd),
                     "encoder.rnn.bias_ih_l0" + suf: (3 * Hd,), "encoder.rnn.bias_hh_l0" + suf: (3 * Hd,)})
    assert {k: tuple(v.shape) for k, v in sd.items() if ".rnn." in k} == want
    opt.seed = 6
    ck = {"model": {k: v.cpu() for k, v in sd.items() if not k.startswith("generator.")},
          "generator": {k[len("generator."):]: v.cpu() for k, v in sd.items() if k.startswith("generator.")}}
    m2 = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, ck)          # strict load of the reference's names
    sd2 = m2.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)
    m2.eval()
    g = torch.Generator().manual_seed(1)
    S, B, K, max_len = 9, 3, 2, 12
    lens = torch.tensor([9, 6, 2])
    src = torch.randint(2, c.vs, (S, B), generator=g)
    for b in range(B):
        src[lens[b]:, b] = 1
    tr = TranslatorMultimodalVI(m2, fields, beam_size=K, n_best=1, max_length=max_len, global_scorer=GNMTGlobalScorer(0.0, 0.0))
    ret = tr.translate_batch(types.SimpleNamespace(src=(src, lens)))
    assert len(ret["predictions"]) == B and all(1 <= len(p[0]) <= max_len for p in ret["predictions"])
    # the decoder's first-position state (right half of cat) against an fp64 GRU cell from the encoder's final h, emb(BOS) and z
    e, bos = m2.engine, 2
    ws = _encode(e, src.to(e.dev), lens, bos)
    torch.cuda.synchronize()
    got = ws.cat.view()[:B, e.d.hp:e.d.hp + H].double().cpu()
    P = {k: v.double().cpu() for k, v in sd.items()}
    h0, z = ws.hn[0].view()[:B, :H].double().cpu(), ws.z32.view()[:B].double().cpu()
    x = torch.cat([P["decoder.embeddings.make_embedding.emb_luts.0.weight"][bos].expand(B, c.emb), z], 1)
    gi = x @ P["decoder.rnn.weight_ih_l0"].t() + P["decoder.rnn.bias_ih_l0"]
    gh = h0 @ P["decoder.rnn.weight_hh_l0"].t() + P["decoder.rnn.bias_hh_l0"]
    r, u = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    assert (got - (n + u * (h0 - n))).abs().max().item() <= 2e-5


def test_gru_with_conditional_is_refused_by_name():
    from variational_mmt_amd.engine import Dims
    with pytest.raises(NotImplementedError, match="GRU.*conditional"):
        Dims(40, 50, 32, 64, 16, 64, 1, True, 0.0, conditional=True, rnn="GRU")
