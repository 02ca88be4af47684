"""Host side of the wide attention keys (d_key up to 576 = 9 x 64; Wikipedia / Reddit: 172 + 172 + 172 = 516):
the TGAT constructor's limit, the state_dict at that width, and learn_base's refusals for TGN, which keep TGN base
training where it was."""
import numpy as np
import pytest
import torch


def _feats(dn, de, V=12, E=20):
    rng = np.random.default_rng(dn + de)
    nf = rng.uniform(-1, 1, (V, dn)).astype(np.float32)
    ef = rng.uniform(-1, 1, (E, de)).astype(np.float32)
    nf[0] = ef[0] = 0
    return nf, ef


def test_tgat_constructs_at_wikipedia_width():
    from tempme_amd.tgat import TGAT
    nf, ef = _feats(172, 172)
    m = TGAT(nf, ef, 20, num_layers=2, n_head=2)
    assert m.model_dim == 516 and m.time_dim == 172
    assert m.fused_tail is False                                 # the tail's choice does not depend on the width
    sd = m.state_dict()
    assert sd["attn_model_list.0.multi_head_target.w_qs.weight"].shape == (516, 516)
    torch.manual_seed(1)
    m2 = TGAT(nf, ef, 20, num_layers=2, n_head=2)
    assert any(not torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    m2.load_state_dict(sd)
    assert sd.keys() == m2.state_dict().keys()
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("dn,de,H", [(192, 192, 4), (171, 171, 3)])
def test_tgat_constructs_up_to_576(dn, de, H):
    from tempme_amd.tgat import TGAT
    nf, ef = _feats(dn, de)
    assert TGAT(nf, ef, 5, num_layers=2, n_head=H).model_dim == 2 * dn + de


def test_tgat_refuses_above_576():
    from tempme_amd.tgat import TGAT
    nf, ef = _feats(200, 200)
    with pytest.raises(NotImplementedError, match="576") as e:
        TGAT(nf, ef, 20, num_layers=2, n_head=2)
    assert "600" in str(e.value)
    nf, ef = _feats(192, 193)                                    # 577: the first width past the ninth register
    with pytest.raises(NotImplementedError, match="576"):
        TGAT(nf, ef, 20, num_layers=2, n_head=1)


def test_learn_base_keeps_its_tgn_refusals():
    from tempme_amd import learn_base
    for extra in ([], ["--n_layer", "3"], ["--n_layer", "1"]):
        with pytest.raises(NotImplementedError) as e:
            learn_base.main(["--base_type", "tgn", "-d", "wikipedia"] + extra)
        msg = str(e.value)
        assert "tgn" in msg and "--n_layer 2" in msg and "2-hop" in msg
    with pytest.raises(NotImplementedError, match="--n_layer 2"):
        learn_base.main(["--base_type", "tgat", "--n_layer", "3", "-d", "wikipedia"])
    # --n_layer 2 gets past the switch for both: the next thing wanted is the data set
    for base in ("tgn", "tgat"):
        with pytest.raises(FileNotFoundError):
            learn_base.main(["--base_type", base, "--n_layer", "2", "-d", "wikipedia", "--data_dir", "no_such_directory"])


def test_header_states_the_limits():
    import os
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "tempme.h")).read()
    assert "d_key <= 576" in text and "feat <= d_key <= 576" in text
    assert "d_key <= 512" in text                                # TGN base training, the remaining gap
