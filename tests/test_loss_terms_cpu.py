"""CPU: the loss settings the model takes from its config (model.LOSS_FIELDS) -- every field arrives as a plain attribute, and a
config that lacks one gets the default of TrainingConfig's own dataclass field.  The constructor itself needs the HIP device, so the
part of it that reads these settings (``_read_loss_settings``, which touches no device) runs here on a stand-in, as the checkpoint
tests of test_center_cpu.py stand in for the model; tests/test_loss_terms_gpu.py looks at the attributes of the real one."""
import dataclasses
import types

import pytest

from prcv2025reid_amd.config import TrainingConfig
from prcv2025reid_amd.model import AUX_TERMS, LOSS_FIELDS, CLIPBasedMultiModalReIDModel

DEFAULTS = {f.name: f.default for f in dataclasses.fields(TrainingConfig)}
# a value per field that is not its default
OTHER = dict(sdm_temperature=0.07, ce_weight=0.5, triplet_weight=0.3, triplet_margin=None, cross_triplet_weight=0.5, cross_triplet_margin=0.2,
             cross_triplet_normalize=False, hc_triplet_weight=0.25, hc_triplet_margin=None, hc_triplet_normalize=False, xbm_weight=0.75,
             xbm_size=64, xbm_margin=0.1, xbm_normalize=False, xbm_start_epoch=0, center_weight=5e-4, center_alpha=0.25,
             center_source='modalities')


def settings_of(config):
    model = types.SimpleNamespace()
    CLIPBasedMultiModalReIDModel._read_loss_settings(model, config)
    return model


def test_the_names_are_config_fields_and_cover_every_term():
    assert len(set(LOSS_FIELDS)) == len(LOSS_FIELDS) and set(LOSS_FIELDS) <= set(DEFAULTS)
    assert set(OTHER) == set(LOSS_FIELDS) and all(OTHER[n] != DEFAULTS[n] for n in LOSS_FIELDS)
    assert [name for name, _ in AUX_TERMS] == ['triplet', 'cross_triplet', 'hc_triplet', 'xbm', 'center']
    for name, count_key in AUX_TERMS:
        assert name + '_weight' in LOSS_FIELDS and DEFAULTS[name + '_weight'] == 0.0
        assert callable(getattr(CLIPBasedMultiModalReIDModel, f'_{name}_term'))


def test_default_config_gives_the_dataclass_defaults():
    model = settings_of(TrainingConfig())
    for n in LOSS_FIELDS:
        assert getattr(model, n) == DEFAULTS[n] and type(getattr(model, n)) is type(DEFAULTS[n]), n
    assert (model.id_head, model.id_scale, model.id_margin) == ('linear', None, None)
    assert model.contrastive_weight == DEFAULTS['contrastive_weight'] == 0.0


def test_every_value_of_a_config_arrives():
    model = settings_of(TrainingConfig(**OTHER, id_head='circle', contrastive_weight=0.3))
    for n in LOSS_FIELDS:
        assert getattr(model, n) == OTHER[n] and type(getattr(model, n)) is type(OTHER[n]), n
    assert (model.id_head, model.id_scale, model.id_margin) == ('circle', 64.0, 0.35) and model.contrastive_weight == 0.3
    model.triplet_weight = 0.0                                   # plain attributes: assignable after construction
    assert model.triplet_weight == 0.0


def test_a_config_without_the_fields_gets_the_defaults():
    """The reference's config knows none of the added losses: a bare namespace constructs with the dataclass defaults (and with the
    reference's own fallback for contrastive_weight, models/model.py:294)."""
    model = settings_of(types.SimpleNamespace())
    for n in LOSS_FIELDS:
        assert getattr(model, n) == DEFAULTS[n], n
    assert (model.id_head, model.id_scale, model.id_margin) == ('linear', None, None)
    assert model.contrastive_weight == 0.1
    part = settings_of(types.SimpleNamespace(xbm_size=128, ce_weight=2.0))
    assert (part.xbm_size, part.ce_weight, part.xbm_weight) == (128, 2.0, 0.0)


def test_the_two_validations_stay():
    with pytest.raises(ValueError, match="center_source must be 'fused' or 'modalities'"):
        settings_of(TrainingConfig(center_source='raw'))
    with pytest.raises(ValueError, match='id_head must be'):
        settings_of(TrainingConfig(id_head='softmax'))
    with pytest.raises(ValueError, match='margin'):
        settings_of(TrainingConfig(id_head='cosface', id_margin=1.5))
