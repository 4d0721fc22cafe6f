"""The CPU oracle (oracle/cpu_ref.py) against golden vectors captured from the reference
(oracle/capture_golden.py).  This is what pins the oracle; the GPU parity tests then compare
the HIP path with the oracle and with the same fixtures."""
import numpy as np
import pytest
import torch

from oracle import cpu_ref
from texocr_amd import synth
from texocr_amd.config import Dims
from conftest import load_golden


def model_of(meta):
    d = Dims(**meta["dims"])
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, meta["weight_seed"]))
    img = torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"]))
    return d, sd, img


def first_divergence(a, b):
    """index of the first step where token rows differ (per row), or T."""
    neq = (a != b)
    T = a.shape[1]
    return np.where(neq.any(1), neq.argmax(1), T)


def test_state_dict_layout_matches_reference():
    meta, _ = load_golden("tiny")
    d = Dims(**meta["dims"])
    ours = [[k, list(s), c] for k, s, c in synth.state_dict_layout(d)]
    assert ours == meta["state_dict_layout"]
    sd = synth.synth_state_dict(d, 7)
    # aliased shared-LN keys are one array
    assert sd["encoder.attn_layers.layers.3.0.weight"] is sd["encoder.attn_layers.layers.0.0.weight"]
    assert sd["decoder.net.attn_layers.layers.5.0.bias"] is sd["decoder.net.attn_layers.layers.0.0.bias"]


def test_tiny_every_stage():
    meta, g = load_golden("tiny")
    d, sd, img = model_of(meta)
    np.testing.assert_allclose(cpu_ref.patch_embed(sd, img).numpy(), g["patch_embed"], atol=2e-6)
    trace = []
    enc = cpu_ref.encode(sd, img, trace)
    np.testing.assert_allclose(enc.numpy(), g["enc"], atol=5e-6)
    # hiddens: x entering each layer's self sub-layer = after the previous layer's mlp sub-layer
    # (sub-layer trace index 2*i-1), last = stack output
    for i in range(1, d.enc_layers):
        np.testing.assert_allclose(trace[2 * i - 1].numpy(), g["enc_hiddens"][i], atol=5e-6)
    np.testing.assert_allclose(trace[-1].numpy(), g["enc_hiddens"][-1], atol=5e-6)
    toks = torch.from_numpy(g["tokens"].astype(np.int64))
    prefix = torch.cat([torch.full((2, 1), d.bos, dtype=torch.long), toks[:, :-1]], 1)
    dtrace = []
    tfl = cpu_ref.decoder_net(sd, prefix, enc, dtrace)
    np.testing.assert_allclose(tfl.numpy(), g["tf_logits"], atol=1e-5)
    for i in range(1, d.dec_layers):
        np.testing.assert_allclose(dtrace[3 * i - 1].numpy(), g["dec_hiddens"][i], atol=1e-5)
    np.testing.assert_allclose(dtrace[-1].numpy(), g["dec_hiddens"][-1], atol=1e-5)
    # cached form == recompute form
    tfc = cpu_ref.teacher_forced_logits_cached(sd, enc, prefix)
    np.testing.assert_allclose(tfc.numpy(), g["tf_logits"], atol=1e-5)
    t_re, l_re = cpu_ref.generate_recompute(sd, img, d.bos, d.eos, meta["max_len"], collect_logits=True)
    t_ca, l_ca = cpu_ref.generate_cached(sd, img, d.bos, d.eos, meta["max_len"], collect_logits=True)
    assert np.array_equal(t_re.numpy(), g["tokens"])
    assert np.array_equal(t_ca.numpy(), g["tokens"])
    np.testing.assert_allclose(l_re.numpy(), g["step_logits"], atol=1e-5)
    np.testing.assert_allclose(l_ca.numpy(), g["step_logits"], atol=1e-5)


def test_cfg1_greedy_tokens_and_logits():
    meta, g = load_golden("cfg1_b4_224x224")
    d, sd, img = model_of(meta)
    enc = cpu_ref.encode(sd, img)
    np.testing.assert_allclose(enc[0].numpy(), g["enc0"], atol=2e-5)
    np.testing.assert_allclose(enc.double().sum((1, 2)).numpy(), g["enc_sum"], rtol=0, atol=2e-2)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, 256, collect_logits=True, enc=enc)
    assert toks.shape == (4, 256)          # eos never fires for all rows -> full length
    assert np.array_equal(toks.numpy(), g["tokens"]), first_divergence(toks.numpy(), g["tokens"])
    assert float(g["margin"].min()) > 5e-5
    np.testing.assert_allclose(logits[:2, :16].numpy(), g["logits_first16"], atol=2e-5)
    np.testing.assert_allclose(logits[:2, -4:].numpy(), g["logits_last4"], atol=5e-5)
    v = torch.gather(logits, 2, torch.from_numpy(g["top5_ids"].astype(np.int64)))
    np.testing.assert_allclose(v.numpy(), g["top5_vals"], atol=5e-5)


def test_cfg1_float64_oracle_matches_reference():
    """The float64 run of the oracle (tests/ref64.py) -- the reference of the shape-matrix GPU tests -- against the fixture captured
    from the reference: tokens equal wherever the fixture's top-1/top-2 margin is >= 1e-4, logits within 1e-4 (the fixture is fp32:
    what is left is its own rounding)."""
    import ref64
    meta, g = load_golden("cfg1_b4_224x224")
    d, sd, img = model_of(meta)
    s64 = ref64.sd64(synth.synth_state_dict(d, meta["weight_seed"]))
    enc = ref64.encode(s64, img)
    assert enc.dtype == torch.float64
    np.testing.assert_allclose(enc[0].numpy(), g["enc0"], atol=1e-4)
    toks, logits = ref64.generate(s64, enc, d.bos, d.eos, 256)
    assert logits.dtype == torch.float64 and toks.shape == (4, 256)
    sure = g["margin"] >= 1e-4
    assert sure.mean() > 0.99
    assert np.array_equal(toks.numpy()[sure], g["tokens"][sure])
    np.testing.assert_allclose(logits[:2, :16].numpy(), g["logits_first16"], atol=1e-4)
    np.testing.assert_allclose(logits[:2, -4:].numpy(), g["logits_last4"], atol=1e-4)
    v = torch.gather(logits, 2, torch.from_numpy(g["top5_ids"].astype(np.int64)))
    np.testing.assert_allclose(v.numpy(), g["top5_vals"], atol=1e-4)
    # the fp32 oracle on the same prefix is within its own rounding of the float64 one (and the fixture tests above stay fp32)
    tf = cpu_ref.decoder_net(sd, torch.cat([torch.full((4, 1), d.bos, dtype=torch.long), toks[:, :15]], 1), cpu_ref.encode(sd, img))
    assert tf.dtype == torch.float32
    assert float((tf.double() - logits[:, :16]).abs().max()) < 1e-4


def test_cfg2_shape_encoder_and_decode():
    meta, g = load_golden("cfg2_b2_224x672")
    d, sd, img = model_of(meta)
    enc = cpu_ref.encode(sd, img)
    assert enc.shape == (2, 589, 256)
    np.testing.assert_allclose(enc[:, ::8].numpy(), g["enc_rows"], atol=2e-5)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, 48, collect_logits=True, enc=enc)
    assert np.array_equal(toks.numpy(), g["tokens"])
    np.testing.assert_allclose(logits[:, :8].numpy(), g["logits_first8"], atol=2e-5)


def test_recompute_mode_matches_reference_cfg1_prefix():
    """The 'reference CPU path' baseline mode (no cache) on the first 12 steps of config 1."""
    meta, g = load_golden("cfg1_b4_224x224")
    d, sd, img = model_of(meta)
    toks = cpu_ref.generate_recompute(sd, img[:2], d.bos, d.eos, 12)
    assert np.array_equal(toks.numpy(), g["tokens"][:2, :12])


def test_pos_ids():
    meta, g = load_golden("posids")
    for H, W, canvas in meta["cases"]:
        ids = cpu_ref.pos_ids(H // 16, W // 16, canvas // 16).numpy()
        assert np.array_equal(ids, g[f"ids_{H}_{W}_{canvas}"])
    lc = meta["live_case"]
    d, sd, img = model_of(lc)
    np.testing.assert_allclose(cpu_ref.encode(sd, img).numpy(), g["enc_32_80_96"], atol=5e-6)


def test_eos_global_break():
    meta, g = load_golden("eos_break")
    d, sd, img = model_of(meta)
    for case in meta["cases"]:
        for gen in (cpu_ref.generate_cached, cpu_ref.generate_recompute):
            t = gen(sd, img, d.bos, case["eos"], meta["max_len"])
            assert t.shape[1] == case["n_steps"], case
            assert np.array_equal(t.numpy(), g[f"tokens_{case['name']}"])
    names = {c["name"]: c for c in meta["cases"]}
    assert names["both"]["n_steps"] < meta["max_len"]       # early global break
    assert names["only_row0"]["n_steps"] == meta["max_len"]  # a finished row keeps generating
    assert names["eos_is_bos"]["n_steps"] == 1


def test_row_stop_is_the_reference_up_to_each_rows_first_eos():
    """stop='row' (build extension; the reference has no such mode): against the tokens captured from the reference's global-break
    loop, every row is identical up to and including its first eos, `pad` behind it, and the loop ends at the same step."""
    meta, g = load_golden("eos_break")
    d, sd, img = model_of(meta)
    for case in meta["cases"]:
        ref_tok = g[f"tokens_{case['name']}"]
        for gen in (cpu_ref.generate_cached, cpu_ref.generate_recompute):
            t = gen(sd, img, d.bos, case["eos"], meta["max_len"], stop="row", pad=d.pad).numpy()
            assert t.shape == ref_tok.shape, case
            for b in range(t.shape[0]):
                if case["eos"] == d.bos:
                    assert (t[b] == d.pad).all()
                    continue
                hits = np.nonzero(ref_tok[b] == case["eos"])[0]
                n = int(hits[0]) + 1 if hits.size else t.shape[1]
                assert np.array_equal(t[b, :n], ref_tok[b, :n]) and (t[b, n:] == d.pad).all(), (case, b)
    # the rewrite on its own, start tokens included in the test (decoder.py:115 looks at the whole output)
    out = torch.tensor([[5, 1, 2, 9, 3, 9], [5, 9, 1, 2, 3, 4], [9, 1, 2, 3, 4, 5], [5, 1, 2, 3, 4, 6]])
    got = cpu_ref.pad_after_eos(out, 2, 9, 0)
    assert got.tolist() == [[2, 9, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2, 3, 4, 6]]


def test_sliding_window_recompute_only():
    meta, g = load_golden("sliding_window")
    d, sd, img = model_of(meta)
    t = cpu_ref.generate_recompute(sd, img, d.bos, d.eos, meta["max_len"])
    assert np.array_equal(t.numpy(), g["tokens"])
    with pytest.raises(ValueError):
        cpu_ref.generate_cached(sd, img, d.bos, d.eos, meta["max_len"])


def test_sampling_distribution():
    meta, g = load_golden("sampling")
    logits = torch.from_numpy(g["logits"])
    filt = cpu_ref.topk_filter(logits)
    assert int((filt[0] > -float("inf")).sum()) == meta["support"] == 99
    np.testing.assert_allclose(cpu_ref.sample_probs(logits, meta["temp"]).numpy(), g["probs"], atol=1e-7)


def test_hybrid_default_factory_every_stage():
    """N1: create_model(config/config.yml) -- ResNetV2 [2,4,6] hybrid embedder, (160, 1008) canvas."""
    meta, g = load_golden("hybrid_b2_32x96")
    d, sd, img = model_of(meta)
    assert d.embed == "hybrid" and d.canvas_hw == (160, 1008) and meta["n_state_dict_keys"] == 372
    p = "encoder.patch_embed.backbone_net"
    x = cpu_ref.std_conv(img, sd[f"{p}.stem.0.weight"], 2)
    x = cpu_ref.group_norm_act(sd, f"{p}.stem.1", x, True)
    x = torch.nn.functional.max_pool2d(cpu_ref._same_pad(x, 3, 2, value=-float("inf")), 3, 2)
    np.testing.assert_allclose(x.numpy(), g["stem"], atol=2e-5)
    f = cpu_ref.resnet_backbone(sd, p, img)
    np.testing.assert_allclose(f.numpy(), g["stage2"], atol=5e-5)
    np.testing.assert_allclose(cpu_ref.hybrid_embed(sd, img).numpy(), g["embed"], atol=5e-5)
    enc = cpu_ref.encode(sd, img, grid_w=d.grid)
    np.testing.assert_allclose(enc.numpy(), g["enc"], atol=5e-5)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, meta["max_len"], collect_logits=True, enc=enc)
    assert np.array_equal(toks.numpy(), g["tokens"])
    np.testing.assert_allclose(logits.numpy(), g["step_logits"], atol=5e-5)


def test_hybrid_default_factory_full_canvas():
    """The default factory's model at its real size: 1x160x1008 canvas, 631 tokens, 32 reference steps (cap_hybrid_full)."""
    meta, g = load_golden("hybrid_b2_160x1008")
    d, sd, img = model_of(meta)
    assert tuple(img.shape) == (2, 1, 160, 1008) and meta["tokens_per_image"] == 631
    np.testing.assert_allclose(cpu_ref.hybrid_embed(sd, img).numpy()[:, ::8], g["embed_every8"], atol=1e-4)
    enc = cpu_ref.encode(sd, img, grid_w=d.grid)
    np.testing.assert_allclose(enc.numpy(), g["enc"], atol=1e-4)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, meta["max_len"], collect_logits=True, enc=enc)
    assert np.array_equal(toks.numpy(), g["tokens"])
    np.testing.assert_allclose(logits.numpy(), g["step_logits"], atol=1e-4)


def test_cfg4_vit_base_encoder_and_decode():
    """G10 / BASELINE config 4: ViT-Base 12L/768d/12h encoder + 6L/768d/12h decoder, B=2, 224x672, 8 reference steps."""
    meta, g = load_golden("cfg4_b2_224x672")
    d, sd, img = model_of(meta)
    assert (d.embed_dim, d.enc_layers, d.dec_layers, d.enc_heads) == (768, 12, 6, 12)
    enc = cpu_ref.encode(sd, img)
    assert enc.shape == (2, 589, 768)
    np.testing.assert_allclose(enc[:, ::16, ::4].numpy(), g["enc_rows"], atol=5e-5)
    np.testing.assert_allclose(enc.double().sum((1, 2)).numpy(), g["enc_sum"], rtol=0, atol=0.05)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, 8, collect_logits=True, enc=enc)
    assert float(g["margin"].min()) > 1e-2                    # a robust fixture: no razor-thin decisions
    assert np.array_equal(toks.numpy(), g["tokens"])
    np.testing.assert_allclose(logits.numpy(), g["step_logits"], atol=5e-5)


def test_cfg2_benchmark_shape_256_steps():
    """The benchmark's own shape for the whole decode: 3x224x672, B=2, 256 reference steps (min margin >= 1e-4)."""
    meta, g = load_golden("cfg2_b2_224x672_t256")
    d, sd, img = model_of(meta)
    assert float(g["margin"].min()) >= 1e-4 and meta["max_len"] == 256
    enc = cpu_ref.encode(sd, img)
    np.testing.assert_allclose(enc[:, ::8].numpy(), g["enc_rows"], atol=2e-5)
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, 256, collect_logits=True, enc=enc)
    assert np.array_equal(toks.numpy(), g["tokens"]), first_divergence(toks.numpy(), g["tokens"])
    v = torch.gather(logits, 2, torch.from_numpy(g["top5_ids"].astype(np.int64)))
    np.testing.assert_allclose(v.numpy(), g["top5_vals"], atol=5e-5)
    np.testing.assert_allclose(logits[:, -4:].numpy(), g["logits_last4"], atol=5e-5)


def test_cfg4_vit_base_64_steps():
    """BASELINE config 4 for 64 reference steps (B=2)."""
    meta, g = load_golden("cfg4_b2_224x672_t64")
    d, sd, img = model_of(meta)
    assert float(g["margin"].min()) >= 1e-4
    toks, logits = cpu_ref.generate_cached(sd, img, d.bos, d.eos, 64, collect_logits=True)
    assert np.array_equal(toks.numpy(), g["tokens"]), first_divergence(toks.numpy(), g["tokens"])
    v = torch.gather(logits, 2, torch.from_numpy(g["top5_ids"].astype(np.int64)))
    np.testing.assert_allclose(v.numpy(), g["top5_vals"], atol=1e-4)
    np.testing.assert_allclose(logits[:, -4:].numpy(), g["logits_last4"], atol=1e-4)


def test_wrapper_fixture_preprocess_and_decode():
    """N3: the oracle on the tensor the reference's wrapper fed its model (hybrid default factory), inside the
    positional table and beyond it (the reference slides its window, decoder.py:99-100: recompute mode only);
    the host-side pieces of the build's wrapper (preprocess, detokenise, process_output) against the same fixture."""
    from PIL import Image
    from texocr_amd.wrapper import preprocess_image
    from texocr_amd.tokenizer import RegExTokenizer, process_output
    import json, os
    meta, g = load_golden("wrapper_160x48")
    d = Dims(**meta["dims"])
    x = preprocess_image(Image.fromarray(g["pixels"]))
    assert np.array_equal(x.numpy(), g["tensor"])             # 48 x 160 are multiples of 16: no padding
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, meta["weight_seed"]))
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    tok = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    for case in meta["cases"]:
        t = cpu_ref.generate_recompute(sd, x[None], d.bos, d.eos, case["max_len"], grid_w=d.grid)   # (160, 1008) canvas: 63 per row
        out = t[0].tolist()[:-1]                              # ocr_model.py:104
        assert out == g[f"tokens_{case['name']}"].tolist(), case["name"]
        assert process_output(tok.decode(out)) == case["text"]
    assert meta["cases"][1]["max_len"] > d.max_len            # the second case really slides


def test_bf16_storage_alone_moves_the_random_hybrid_backbone_by_a_fifth():
    """What the bf16 engine's ~20 % deviation on hybrid-embedder features (random weights) is made of: rounding every stored
    tensor of the 45 conv / GroupNorm layers to bfloat16 on the CPU, all arithmetic in fp32 (cpu_ref.resnet_backbone with
    q=bf16_round), moves the embedder output by the same fifth.  It is the sensitivity of this randomly weighted network to
    8-bit mantissas, not a property of the HIP kernels (tests/test_gpu_parity.py compares the GPU with THIS emulation)."""
    from texocr_amd.config import reference_config
    d = Dims.from_config(reference_config())
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, 9))
    img = torch.from_numpy(synth.synth_images(3, 1, 64, 320, seed=31))
    e32 = cpu_ref.hybrid_embed(sd, img)
    e16 = cpu_ref.hybrid_embed(sd, img, cpu_ref.bf16_round)
    rel = float((e16 - e32).abs().mean() / e32.abs().mean())
    assert 0.08 < rel < 0.35, rel
    # rounding ONLY the input pixels to bf16 (everything else fp32) already moves it by several per cent: no choice of which tensors to
    # store as bf16 helps -- why the bf16 engine keeps this backbone in fp32 (engine.hip: bk_fp32)
    f32 = cpu_ref.resnet_backbone(sd, "encoder.patch_embed.backbone_net", img)
    fin = cpu_ref.resnet_backbone(sd, "encoder.patch_embed.backbone_net", cpu_ref.bf16_round(img))
    assert float((fin - f32).abs().mean() / f32.abs().mean()) > 0.03
    # one rounding alone is ~2^-9: the backbone amplifies it by well over an order of magnitude
    one = float((cpu_ref.bf16_round(e32) - e32).abs().mean() / e32.abs().mean())
    assert one < 0.004 and rel > 20 * one


def test_ragged_prefix_mask_fixture():
    """decoder.generate(start_tokens (B,T0), mask=) and decoder.net(x, mask=) of the reference (decoder.py:95-101,112; attention.py:130-155:
    -FLT_MAX fill where query or key is padding, a fully masked query row softmaxes uniformly over all keys): the oracle reproduces
    the captured tokens, every step's logits and net()'s logits at EVERY position, padded ones included."""
    meta, g = load_golden("ragged_prefix")
    d = Dims(**meta["dims"])
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, meta["weight_seed"]))
    img = torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"]))
    start = torch.from_numpy(g["start"].astype(np.int64))
    mask = torch.from_numpy(g["mask"])
    t, l = cpu_ref.generate_recompute(sd, img, d.bos, None, meta["max_len"], collect_logits=True, start_tokens=start, mask=mask)
    assert np.array_equal(t.numpy(), g["tokens"])
    assert float((l - torch.from_numpy(g["step_logits"])).abs().max()) < 1e-5
    net = cpu_ref.decoder_net(sd, start, cpu_ref.encode(sd, img), mask=mask)
    assert float((net - torch.from_numpy(g["net_logits"])).abs().max()) < 1e-5
    # without the mask the same start tokens decode differently (the fixture pins something)
    plain = cpu_ref.generate_recompute(sd, img, d.bos, None, meta["max_len"], start_tokens=start)
    assert np.array_equal(plain.numpy(), g["tokens_unmasked"]) and not np.array_equal(plain.numpy(), g["tokens"])
