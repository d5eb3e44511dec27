"""The one precision rule of the "high" modes (splatter360_amd/precision.py), on the CPU: the three operator modules expose the
same PRECISIONS, "torch" follows torch.get_float32_matmul_precision() at call time, and the six error messages — three operators,
three install options — are, character for character, the ones each module produced while it had a checker of its own."""
import pytest
import torch

from splatter360_amd import plugin, precision, qkv_attention as qa, transformer_ffn as tf, window_attention as wa

OPERATOR_MESSAGES = {
    "window_attention": "window_attention knows the precisions ['highest', 'high'], got precision='fast'",
    "qkv_attention": "qkv_attention knows the precisions ['highest', 'high'], got precision='fast'",
    "ffn_tail": "ffn_tail knows the precisions ['highest', 'high'], got precision='fast'",
}
OPTION_MESSAGES = {
    "window_attention_precision": "window_attention_precision is one of ['highest', 'high', 'torch'], got 'fast'",
    "unet_attention_precision": "unet_attention_precision is one of ['highest', 'high', 'torch'], got 'fast'",
    "transformer_ffn_precision": "transformer_ffn_precision is one of ['highest', 'high', 'torch'], got 'fast'",
}


def _message(call) -> str:
    with pytest.raises(ValueError) as caught:
        call()
    return str(caught.value)


def test_the_three_modules_expose_one_precisions_object():
    assert wa.PRECISIONS is qa.PRECISIONS is tf.PRECISIONS is precision.PRECISIONS
    assert precision.PRECISIONS == ("highest", "high")
    assert wa.resolve_precision is precision.resolve


def test_resolve_follows_torch_at_call_time():
    assert precision.resolve("highest") == "highest" and precision.resolve("high") == "high"
    assert _message(lambda: precision.resolve("medium")) == OPERATOR_MESSAGES["window_attention"].replace("fast", "medium")
    before = torch.get_float32_matmul_precision()
    try:
        for setting, want in (("highest", "highest"), ("high", "high"), ("medium", "high")):
            torch.set_float32_matmul_precision(setting)
            assert precision.resolve("torch") == wa.resolve_precision("torch") == want
    finally:
        torch.set_float32_matmul_precision(before)
    assert torch.get_float32_matmul_precision() == before


def test_an_operator_s_refusal_is_worded_as_before():
    for name, want in OPERATOR_MESSAGES.items():
        assert _message(lambda: precision.check(name, "fast")) == want
    # through the operators themselves: refused before any tensor is touched
    assert _message(lambda: wa.full_attention(None, None, None, precision="fast")) == OPERATOR_MESSAGES["window_attention"]
    assert _message(lambda: qa.qkv_attention(None, 1, precision="fast")) == OPERATOR_MESSAGES["qkv_attention"]
    assert _message(lambda: tf.ffn_tail_forward(*[None] * 8, precision="fast")) == OPERATOR_MESSAGES["ffn_tail"]
    assert _message(lambda: tf.scratch_bytes(1, False, "fast")) == OPERATOR_MESSAGES["ffn_tail"]
    assert _message(lambda: precision.check("ffn_tail", None)) == OPERATOR_MESSAGES["ffn_tail"].replace("'fast'", "None")
    for good in precision.PRECISIONS:
        assert precision.check("ffn_tail", good) == good


def test_an_install_option_s_refusal_is_worded_as_before():
    for option, want in OPTION_MESSAGES.items():
        assert _message(lambda: precision.seam_option(option, "fast")) == want
        for good in (*precision.PRECISIONS, "torch"):
            assert precision.seam_option(option, good) == good
    # through the install functions: refused before anything is installed
    assert _message(lambda: plugin.install_window_attention(precision="fast")) == OPTION_MESSAGES["window_attention_precision"]
    assert _message(lambda: plugin.install_unet_attention(precision="fast")) == OPTION_MESSAGES["unet_attention_precision"]
    assert _message(lambda: plugin.install_transformer_ffn(precision="fast")) == OPTION_MESSAGES["transformer_ffn_precision"]
