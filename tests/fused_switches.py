"""Every module-level optimisation switch of ``monosowa_amd`` that has a plain-PyTorch (module-by-module) alternative, and a
context manager that sets all of them to the optimised or to the plain value and restores them afterwards.

Each entry is (module, name, shipped value, plain value).  ``fused_switches(on)`` asserts that every listed switch still
exists before it sets one: a renamed switch must fail loudly, not turn the comparison into a no-op."""
import contextlib
import importlib

SWITCHES = (
    # backbone
    ("monosowa_amd.monodetr.backbone", "AFFINE_IN_KERNEL", True, False),
    ("monosowa_amd.monodetr.backbone", "CACHE_SCALE_SHIFT", True, False),
    ("monosowa_amd.monodetr.backbone", "CONV1X1_EPILOGUE", 3, 0),
    ("monosowa_amd.monodetr.backbone", "CONV1X1_SCALED_GRAD", 1, 0),
    ("monosowa_amd.monodetr.backbone", "FOLD_DOWNSAMPLE_SHIFT", True, False),
    ("monosowa_amd.monodetr.backbone", "FUSED_FROZEN_DS", True, False),
    ("monosowa_amd.monodetr.backbone", "FUSED_FROZEN_TAIL", True, False),
    ("monosowa_amd.monodetr.backbone", "FUSED_STEM", True, False),
    ("monosowa_amd.monodetr.position_encoding", "CACHE_ALL_VALID", True, False),
    # transformer
    ("monosowa_amd.monodetr.depthaware_transformer", "ENCODER_BLOCKS", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "LEVEL_EMBED_IN_BLOCK", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "MERGE_SA_PROJ", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "SELF_ATTN_HIP", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "BROADCAST_POS", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "FUSED_REFINE", True, False),
    ("monosowa_amd.monodetr.depthaware_transformer", "MERGE_VALUE_PROJ", True, False),
    ("monosowa_amd.ms_deform_attn", "MERGED_PROJ", True, False),
    ("monosowa_amd.ms_deform_attn", "MASK_IN_KERNEL", True, False),
    ("monosowa_amd.ms_deform_attn_func", "SAVE_PROLOGUE", True, False),
    ("monosowa_amd.encoder_block", "MERGED_PROJ", True, False),
    ("monosowa_amd.encoder_block", "FUSED_BIAS_SUMS", True, False),
    ("monosowa_amd.token_linear", "FAST_LINEAR", True, False),
    ("monosowa_amd.token_linear", "USE_SUM_SLICES", True, False),
    ("monosowa_amd.token_linear", "SMALL_WGRAD_KERNEL", 1, 0),
    ("monosowa_amd.pointwise", "USE_RELU_MASK", True, False),
    ("monosowa_amd.pointwise", "COLSUM_LEVELS_ONE_LAUNCH", 1, 0),
    ("monosowa_amd.pointwise", "DDN_EAGER_BACKWARD", True, False),
    # depth predictor, heads
    ("monosowa_amd.monodetr.depth_predictor", "FUSED_EXPECTATION", True, False),
    ("monosowa_amd.monodetr.monodetr", "MERGE_HEADS", True, False),
    ("monosowa_amd.monodetr.monodetr", "FUSED_HEAD_TAIL", True, False),
    ("monosowa_amd.monodetr.monodetr", "REUSE_BBOX_RAW", True, False),
    ("monosowa_amd.monodetr.monodetr", "USE_LAYER_TENSORS", True, False),
    # matcher and criterion
    ("monosowa_amd.monodetr.matcher", "BLOCK_COST", True, False),
    ("monosowa_amd.monodetr.matcher", "FUSED_COST", True, False),
    ("monosowa_amd.monodetr.matcher", "DEVICE_LSAP", True, False),
    ("monosowa_amd.monodetr.criterion", "FUSED_FOCAL", True, False),
    ("monosowa_amd.monodetr.criterion", "FUSED_MATCHED", True, False),
    ("monosowa_amd.monodetr.losses", "FUSED_DDN", True, False),
    # detection extraction
    ("monosowa_amd.helpers.decode_helper", "DEVICE_KERNEL", True, False),
)


def resolved():
    """[(module object, name, shipped, plain)]; fails on a switch that no longer exists."""
    out = []
    for mod_name, name, shipped, plain in SWITCHES:
        mod = importlib.import_module(mod_name)
        assert hasattr(mod, name), "%s.%s is gone: update tests/fused_switches.py" % (mod_name, name)
        out.append((mod, name, shipped, plain))
    return out


@contextlib.contextmanager
def fused_switches(on):
    """on=True: every listed switch at its shipped (optimised) value; on=False: every one at its plain-PyTorch value."""
    table = resolved()
    saved = [(mod, name, getattr(mod, name)) for mod, name, _, _ in table]
    try:
        for mod, name, shipped, plain in table:
            setattr(mod, name, shipped if on else plain)
        yield
    finally:
        for mod, name, val in saved:
            setattr(mod, name, val)
