"""GPU (-m gpu): the activation epilogue (hsp_conv1d_args.act = HSP_ACT_ACT1D) in the model.  SynthesizerTrn.infer at 2 x 1 s with
the form on (HSP_EPI_ACT=1, hip_layers.EPI_ACT) equals the form off under torch.equal -- the fused launch is the same sum
and the same activation arithmetic as the two launches it replaces -- and the hooks report what ran: fewer stand-alone
activation launches, exactly as many as conv launches that carry the value."""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


def _model(meta, device):
    from megatts2_hierspeechpp_amd import synth
    from megatts2_hierspeechpp_amd.hip_layers import finalize
    mod = H.build_module(meta)
    sd = H.synth_sd(meta)
    pre = meta["prefix"] + "." if meta["prefix"] else ""
    for k, v in mod.state_dict().items():
        if k not in sd:
            sd[k] = torch.from_numpy(synth.synth_tensor(pre + k, tuple(v.shape), meta["seed"]))
    mod.load_state_dict(sd, strict=True)
    finalize(mod, device)
    return mod


def test_synthesizer_infer_is_unchanged_by_the_form(device, monkeypatch):
    from megatts2_hierspeechpp_amd import functional as Fh
    from megatts2_hierspeechpp_amd import hip_layers as HL
    meta, a = H.load_fixture("infer_config1")
    mod = _model(meta, device)
    B, T = 2, 50                                   # 2 x 1 s at 50 frames per second
    r = np.random.default_rng(23)
    d = lambda shape, scale=1.0: torch.from_numpy((scale * r.standard_normal(shape)).astype(np.float32)).to(device)
    per = a["f0"].shape[-1] // a["w2v"].shape[2]
    mel, w2v = d((B,) + a["mel"].shape[1:-1] + (T,)), d((B,) + a["w2v"].shape[1:-1] + (T,))
    f0, noise = d((B,) + a["f0"].shape[1:-1] + (per * T,), 0.5), d((B,) + a["noise"].shape[1:-1] + (T,))
    fused, acts = [], []
    monkeypatch.setattr(HL, "LAUNCH_HOOK", lambda kind, flops, nbytes, e0, e1, arg:
                        fused.append((arg.Cin, arg.K, arg.dil, arg.ncols)) if getattr(arg, "act", 0) == HL.L.ACT_ACT1D else None)
    monkeypatch.setattr(Fh, "ACT_HOOK", lambda nb, e0, e1: acts.append(nb))
    outs, counts = [], []
    for on in (False, True):
        monkeypatch.setattr(HL, "EPI_ACT", on)
        del fused[:], acts[:]
        with torch.no_grad():
            o, e_ = mod.infer(mel, w2v, torch.tensor([T, T], device=device), f0, noise=noise)
        torch.cuda.synchronize()
        outs.append((o.clone(), e_.clone()))
        counts.append((len(fused), len(acts)))
    print(f"epi_act model: fused conv launches off / on = {counts[0][0]} / {counts[1][0]}, stand-alone activations "
          f"{counts[0][1]} / {counts[1][1]}; fused shapes (Cin, K, dil, L): {sorted(set(fused))}")
    assert counts[0][0] == 0 and counts[1][0] > 0
    assert all(cin <= 64 for cin, _, _, _ in fused)
    assert counts[0][1] - counts[1][1] == counts[1][0]        # every fused launch is one activation launch less
    assert torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
