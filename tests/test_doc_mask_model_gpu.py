"""``Llama.set_document_mask`` on the MI355X through the model's attention routes (full fine-tune and LoRA
at head dim 128 and 32, one case under checkpointed recompute): loss and parameter gradients of the HIP
path against the same model's CPU-reference route with the same tables, at the tolerances
tests/test_model_gpu.py::test_train_step_matches_reference_path uses for that comparison without
documents (loss 2e-2 relative, gradients 6e-2 relative Frobenius)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(preset, lora, ckpt, gpu):
    from mxllm.models import Llama, get_config

    cfg = get_config(preset)
    m = Llama(cfg, device=gpu, lora_r=lora, seed=5, activation_checkpointing=ckpt)
    if lora:
        with torch.no_grad():
            for mod in m.modules():
                if getattr(mod, "lora_r", 0):
                    for blk in mod.lora_b_blocks():
                        blk.normal_(0, 0.02)
            m.sync_adapters_()
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(3, cfg.vocab_size, (2, 192), generator=g)
    ids[0, [40, 63, 64, 130]] = cfg.eos_id  # documents ending at a tile edge and inside tiles
    ids[1, [0, 100]] = cfg.eos_id
    return m, ids.to(gpu)


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("preset,lora,ckpt", [("tiny-d128", 0, False), ("tiny-d128", 16, False), ("tiny", 0, False),
                                              ("tiny", 16, False), ("tiny-d128", 0, True)])
def test_document_mask_train_step_matches_reference_path(gpu, preset, lora, ckpt, monkeypatch):
    m, ids = _model(preset, lora, ckpt, gpu)
    m.train()
    m.set_document_mask(m.cfg.eos_id)
    loss = m(ids, ids)
    loss.backward()
    g_native = {n: p.grad.float().clone() for n, p in m.named_parameters() if p.requires_grad}
    m.zero_grad(set_to_none=True)
    monkeypatch.setenv("MXLLM_REFERENCE_OPS", "1")
    loss_ref = m(ids, ids)
    loss_ref.backward()
    assert abs(loss.item() - loss_ref.item()) < 2e-2 * max(1, abs(loss_ref.item()))
    for n, p in m.named_parameters():
        if p.requires_grad:
            e = _rel(g_native[n], p.grad)
            assert e < 6e-2, (n, e)


def test_document_mask_changes_the_loss(gpu):
    m, ids = _model("tiny-d128", 0, False, gpu)
    with torch.no_grad():
        plain = m(ids, ids).item()
        m.set_document_mask(m.cfg.eos_id)
        masked = m(ids, ids).item()
    assert masked != plain
