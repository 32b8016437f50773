"""GPU: compute_loss with every auxiliary term on (model.AUX_TERMS) on the tiny frozen model and a batch of 8 instances (4 identities
x 2, every modality present): the keys of the loss dict and their order, the order of the float additions into total_loss (bit for
bit), and that with every weight 0 nothing of a term exists."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE_KEYS = ['total_loss', 'ce_loss', 'sdm_loss', 'contrastive_loss', 'ce_valid_cnt']
ALL_KEYS = BASE_KEYS + ['triplet_loss', 'triplet_active_cnt', 'cross_triplet_loss', 'cross_triplet_active_cnt', 'hc_triplet_loss',
                        'hc_triplet_active_cnt', 'xbm_loss', 'xbm_active_cnt', 'center_loss', 'center_valid_cnt']
WEIGHTS = dict(triplet_weight=0.3, cross_triplet_weight=0.5, hc_triplet_weight=0.3, xbm_weight=0.5, center_weight=5e-4)


@pytest.mark.parametrize('center_source', ['fused', 'modalities'])
def test_every_term_on_keys_and_addition_order(center_source):
    from helpers import load_case, case_inputs
    from prcv2025reid_amd.model import LOSS_FIELDS
    from prcv2025reid_amd.synthetic import synthetic_batch
    from test_model_gpu import build_model
    z, meta = load_case('tiny_train_frozen')
    cfg, arch, state, _, _ = case_inputs(meta)
    over = dict(WEIGHTS, xbm_size=64, xbm_start_epoch=0, center_source=center_source, sdm_weight_warmup_epochs=0)
    model = build_model(meta, state, True, **over)
    model.contrastive_weight = 0.1
    for n in LOSS_FIELDS:                                        # the real constructor: every field arrived as a plain attribute
        assert getattr(model, n) == over.get(n, getattr(model.config, n)), n
    batch = synthetic_batch(4, 2, arch, seed=7, mask_drop=0.0, num_classes=int(meta['num_classes']))
    images = {m: t.cuda() for m, t in batch['images'].items()}
    masks = {m: t.cuda() for m, t in batch['modality_mask'].items()}
    labels = batch['person_id'].cuda()
    assert labels.shape == (8,) and all(bool((t > 0).all()) for t in masks.values())

    # (c) every weight 0 (assigned after construction): the five keys of the reference, no memory and no table
    for n in WEIGHTS:
        setattr(model, n, 0.0)
    out = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
    assert list(out) == BASE_KEYS
    assert model.xbm_memory is None and model.centers is None

    # (a), (b) every term on
    for n, w in WEIGHTS.items():
        setattr(model, n, w)
    out = model.compute_loss(model(images=images, texts=batch['texts'], modality_masks=masks), labels)
    assert list(out) == ALL_KEYS
    w_ce, w_sdm = model.ce_weight, model.contrastive_weight
    assert w_ce > 0 and w_sdm > 0
    want = (((((w_ce * out['ce_loss'] + w_sdm * out['sdm_loss']) + 0.3 * out['triplet_loss']) + 0.5 * out['cross_triplet_loss'])
             + 0.3 * out['hc_triplet_loss']) + 0.5 * out['xbm_loss']) + 5e-4 * out['center_loss']
    assert torch.equal(out['total_loss'], want), (float(out['total_loss'].detach()), float(want.detach()))
    for k in ('sdm_loss', 'triplet_loss', 'cross_triplet_loss', 'hc_triplet_loss', 'xbm_loss', 'center_loss'):
        assert float(out[k].detach()) > 0, k                     # every term is live: the sum above is not one of zeros
    for k in ALL_KEYS[6::2] + ['ce_valid_cnt']:
        assert int(out[k]) > 0, k
    assert out['contrastive_loss'] is out['sdm_loss']
    assert model.xbm_memory is not None and model.xbm_memory.capacity == 64 and model.centers is not None
    out['total_loss'].backward()
    assert float(model.lora_arena.grad.abs().max()) > 0
