"""MI355X-native MonoDETR forward/backward path for MonoSOWA (gfx950 HIP kernels behind the
reference's MultiScaleDeformableAttention operator boundary)."""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "Detector":                  # the public inference API (monosowa_amd/detector.py); imported on first use
        from .detector import Detector
        return Detector
    if name == "StepHistory":               # the per-step training record (monosowa_amd/history.py)
        from .history import StepHistory
        return StepHistory
    if name == "LabelAudit":                # the per-label disagreement record (monosowa_amd/label_audit.py)
        from .label_audit import LabelAudit
        return LabelAudit
    if name == "Teacher":                   # the mean-teacher path of the train loop (monosowa_amd/teacher.py)
        from .teacher import Teacher
        return Teacher
    if name == "LabelMemory":               # the label memory of self-training (monosowa_amd/teacher_memory.py)
        from .teacher_memory import LabelMemory
        return LabelMemory
    if name == "TemplateFitter":            # the template-pose search behind the first pseudo-labels (monosowa_amd/template_fit.py)
        from .template_fit import TemplateFitter
        return TemplateFitter
    if name in ("ObjectLifter", "LiftResult", "lift_config", "lift_host"):   # depth map and masks to object clouds (monosowa_amd/lift.py)
        from . import lift
        return getattr(lift, name)
    if name in ("ObjectTracker", "TrackResult", "track_config", "track_host"):   # centres to tracks, moving flags, headings (monosowa_amd/track.py)
        from . import track
        return getattr(track, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
