"""GPU: onmt.Optim("sgd" | "adagrad" | "adadelta") through the trainer surface: the HIP update against its torch twin (`Optim.torch_dense`:
torch.optim on the arena views) within the kernel bound of tests/test_gpu_optim_methods.py, the engine's flags, the stand-in's torch-shaped state.
The twin's update takes the gradient arena of the HIP model's step, not a backward of its own: two backward passes over one batch differ by
float-atomic noise (tests/test_gpu_row_adam.py), and Adagrad's first step, g / (|g| + 1e-10), turns that noise into a sign wherever a gradient sits
at the noise floor -- two runs of one build gave 3e-8 and 6.2e-6 for adagrad with a backward each."""
import types

import pytest
import torch

from oracle import vi1_oracle as O
from tests.test_gpu_onmt_surface import _Batch, _Vocab, _opt
from tests.test_gpu_optim_methods import CLS, FP32_ERR, KEYS, _err

pytestmark = pytest.mark.gpu
LR = {"sgd": 0.1, "adagrad": 0.01, "adadelta": 1.0}


@pytest.mark.parametrize("method", ("sgd", "adagrad", "adadelta"))
def test_hip_update_through_the_onmt_surface(method, tmp_path):
    import variational_mmt_amd
    onmt = variational_mmt_amd.install_as_onmt()
    c = O.Cfg(vs=43, vt=47, emb=16, hid=32, z=8, img=2048, layers=1, brnn=True)
    p = O.init_params(c, seed=4)
    batches = [_Batch(O.synth_batch(c, 7, 6, 8, n_img=20, seed=100 + i, fixed_len=False), "cuda") for i in range(3)]
    table = O.synth_batch(c, 7, 6, 8, n_img=20, seed=100, fixed_len=False)["table"].numpy()
    fields = {"src": types.SimpleNamespace(vocab=_Vocab(c.vs, False)), "tgt": types.SimpleNamespace(vocab=_Vocab(c.vt, True))}
    opt = _opt(c, tmp_path)

    def make(torch_dense):
        model = onmt.ModelConstructor.make_vi_model_mmt(opt, fields, True, None)
        model.load_state_dict(dict(p))
        optim = onmt.Optim(method, LR[method], 5.0)
        optim.torch_dense = torch_dense
        optim.set_parameters(model.parameters())
        return model, optim
    (model, optim), (twin, twin_optim) = make(False), make(True)
    loss = onmt.VILoss.NMTVIModel1LossCompute(model.generator, fields["tgt"].vocab)
    trainer = onmt.TrainerMultimodal(model, loss, loss, optim, 0, 32, "text", "sents", 1, train_img_feats=table, valid_img_feats=table,
                                     multimodal_model_type="vi-model1", model_opt=opt, fields=fields)
    eng = model.engine
    start = eng.flat_p[:eng.n_opt].cpu()
    # one training step; the twin applies torch's update to the same parameters and the same gradient (module docstring)
    trainer.train(batches[:1], 1, None)
    twin.engine.flat_g.copy_(eng.flat_g)
    twin_optim.step()
    a, b = eng.flat_p[:eng.n_opt].cpu(), twin.engine.flat_p[:eng.n_opt].cpu()
    e = _err(a, b)
    print("%s: HIP update against the torch twin, p: %.3g" % (method, e))
    assert e <= 4 * FP32_ERR[(method, "p")] and not torch.equal(a, start), e
    # the compute shadows the update left are what a full repack of its parameters gives, bit for bit
    left = {k: buf.view().clone() for k, buf in eng.sh.items()}
    assert not eng.shadows_dirty
    eng.shadows_dirty = True
    eng.refresh_shadows(eng.stream())
    torch.cuda.synchronize()
    assert all(torch.equal(left[k], buf.view()) for k, buf in eng.sh.items())
    for bt in batches[1:]:
        trainer.train([bt], 1, None)
    eng.check_async_errors()
    assert not getattr(eng, "dense_optimizer", False) and eng.seq_fallbacks == 0 and eng.step_count == 3
    assert eng.rows_active() == (method != "adadelta")
    # state_dict() has torch's own layout: it loads into the genuine class over CPU copies and holds the arena's state
    cpu = [torch.nn.Parameter(q.detach().cpu().clone()) for q in optim.params]
    real = CLS[method](cpu, lr=LR[method])
    real.load_state_dict(optim.optimizer.state_dict())
    assert method == "sgd" or eng.flat_m.any()
    for q, q_cpu in zip(optim.params, cpu):
        off, shp = eng.offsets[q._vmmt_name]
        for key, flat in zip(KEYS[method] if q._vmmt_name in eng.grads else (), (eng.flat_m, eng.flat_v)):
            assert torch.equal(real.state[q_cpu][key], flat[off:off + q.numel()].view(*shp).cpu()), (q._vmmt_name, key)
    # set_parameters starts a NEW optimiser (Optim.py:56-67): state zeroed, Adagrad's `sum` at adagrad_accum, step 0
    onmt.Optim(method, LR[method], 5.0, adagrad_accum=0.1).set_parameters(model.parameters())
    assert eng.step_count == 0 and not eng.flat_v.any() and torch.equal(eng.flat_m, torch.full_like(eng.flat_m, 0.1 if method == "adagrad" else 0.0))
