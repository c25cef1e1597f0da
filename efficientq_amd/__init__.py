"""efficientq_amd -- MI355X-native layer-wise PTQ calibration (the hot path of rongzhao-zhang/EfficientQ).

    csrc/            hand-written HIP kernels + the C ABI (include/effq_hip.h) -> libeffq_hip.so
    _lib, hip_ops    ctypes binding and tensor-level front end (no CPU fallback): HipOps holds the calibration wrappers
    ops_base, ops_window, ops_seg, ops_prep
                     the handle and the sliding-window, validation and prep wrappers HipOps is composed from
    qconv            PTQConv / EfficientQConvHIP (reference class contract)
    unet             UResQ host graph (reference module tree / state_dict keys)
    calibrate        do_ptq orchestrator, BN folding, attention-mask pyramid
    config           CLI / YAML surface, factories, the shipped BraTS / LiTS net definitions
    entrance         `python -m efficientq_amd.entrance ptq ...`
    score, ops_score the `score` mission: finished label maps against labels on the scan's grid, and its two device calls
    mixed            per-layer mixed-precision search harness
    synth            seeded synthetic volumes / random-init networks
"""
__version__ = "0.1.0"
