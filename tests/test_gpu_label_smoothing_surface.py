"""GPU: -label_smoothing through the reference's Python surface.  NMTVIModel1LossCompute(label_smoothing=0.1) constructs (on the commit before
this feature its `assert label_smoothing == 0.0` fails here); one update through TrainerMultimodal / NMTVIModel / sharded_compute_loss returns
statistics with the meanings the reference executes -- `nmt_loss` the smoothed KL-divergence sum, `elbo_loss` minus the summed target
log-likelihood alone (onmt/VILoss.py:243-244,479-480), token counts unchanged -- and monolithic_compute_loss (validation: z = mu, dropout 0)
reports the oracle's smoothed sum of the same batch in evaluation mode."""
import types

import pytest
import torch

from oracle import vi1_oracle as O
from tests.test_gpu_label_smoothing_step import smoothed_kld
from tests.test_gpu_onmt_surface import _Batch, _opt, _Vocab

pytestmark = pytest.mark.gpu
EPS = 0.1


def test_label_smoothing_through_the_onmt_surface(tmp_path):
    import variational_mmt_amd
    onmt = variational_mmt_amd.install_as_onmt()
    c = O.Cfg(vs=43, vt=47, emb=16, hid=32, z=8, img=2048, layers=1, brnn=True)
    p = O.init_params(c, seed=4)
    B, S, T = 7, 6, 8
    bt = O.synth_batch(c, B, S, T, n_img=20, seed=100, fixed_len=False)
    fields = {"src": types.SimpleNamespace(vocab=_Vocab(c.vs, False)), "tgt": types.SimpleNamespace(vocab=_Vocab(c.vt, True))}
    opt = _opt(c, tmp_path)
    model = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None)
    model.load_state_dict({k: v for k, v in p.items()})
    train_loss = onmt.VILoss.NMTVIModel1LossCompute(model.generator, fields["tgt"].vocab, label_smoothing=EPS)
    valid_loss = onmt.VILoss.NMTVIModel1LossCompute(model.generator, fields["tgt"].vocab, label_smoothing=EPS)
    with pytest.raises(ValueError):
        onmt.VILoss.NMTVIModel1LossCompute(model.generator, _Vocab(2, False), label_smoothing=EPS)      # eps / (V - 2)
    optim = onmt.Optim("adam", 0.002, 5.0, lr_decay=0.5, start_decay_at=8)
    optim.set_parameters(model.parameters())
    table, img = bt["table"], bt["table"][bt["indices"]]
    trainer = onmt.TrainerMultimodal(model, train_loss, valid_loss, optim, 0, 32, "text", "sents", 1, train_img_feats=table.numpy(),
                                     valid_img_feats=table.numpy(), multimodal_model_type="vi-model1", model_opt=opt, fields=fields)
    stats = trainer.train([_Batch(bt, "cuda")], 1, None)
    eps_z = model.engine.workspace(B, S, T - 1).eps.view().cpu().clone()
    with torch.no_grad():
        r = O.forward(p, c, bt["src"], bt["src_len"], bt["tgt"], img, eps_z, True)
        Lo, kld = O.loss(p, c, r, bt["tgt"], img), float(smoothed_kld(p, c, r, bt["tgt"], EPS))
    print("train: nmt", stats.nmt_loss, kld, "elbo", stats.elbo_loss, float(Lo["nll"]))
    assert abs(stats.nmt_loss - kld) <= 3e-5 * abs(kld)
    assert abs(stats.elbo_loss - float(Lo["nll"])) <= 3e-5 * abs(float(Lo["nll"]))
    assert stats.n_words == Lo["n_words"] and stats.n_correct == Lo["n_correct"]
    # validation of the same batch with the updated parameters: evaluation mode (z = mu), monolithic_compute_loss
    vs = trainer.validate([_Batch(bt, "cuda")])
    p1 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r = O.forward(p1, c, bt["src"], bt["src_len"], bt["tgt"], img, None, False)
        Lo, kld = O.loss(p1, c, r, bt["tgt"], img), float(smoothed_kld(p1, c, r, bt["tgt"], EPS))
    print("valid: nmt", vs.nmt_loss, kld, "elbo", vs.elbo_loss, float(Lo["nll"]))
    assert abs(vs.nmt_loss - kld) <= 3e-5 * abs(kld)
    assert abs(vs.elbo_loss - float(Lo["nll"])) <= 3e-5 * abs(float(Lo["nll"]))
    assert vs.n_words == Lo["n_words"]
