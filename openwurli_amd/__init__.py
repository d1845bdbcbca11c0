"""openwurli-hip: MI355X (gfx950) render core for the OpenWurli DSP hot path.

The product is the C-ABI library ``openwurli_amd/lib/libopenwurli_hip.so`` (declared in
``include/openwurli_hip.h``).  This package is a thin ctypes host mirror of the reference's
``WurliEngine`` / ``Voice::render_note`` API over that library.  There is no CPU fallback:
importing works anywhere, constructing an engine without the built library or without a
HIP device raises.
"""
from .binding import load_library, library_path, OwError  # noqa: F401
from .engine import WurliEngine, EnginePool, VoiceState, render_note, batch_render, normalize_scale, tremolo_prefetch, tremolo_configure, tremolo_export, tremolo_import  # noqa: F401
from . import features  # noqa: F401
from . import alias_audit  # noqa: F401
from . import midi_render  # noqa: F401
from . import calibrate  # noqa: F401
from . import preamp_bench  # noqa: F401
from . import render_poly  # noqa: F401
from . import centroid_track  # noqa: F401
from . import intermod_audit  # noqa: F401
from . import overshoot  # noqa: F401
from . import pump  # noqa: F401
from . import pump_fit  # noqa: F401
from . import pickup_law  # noqa: F401
from . import bark_audit  # noqa: F401
from . import mlp  # noqa: F401
from .mlp import MlpWeights  # noqa: F401
from . import mlp_train  # noqa: F401
from . import harmonics  # noqa: F401
from . import residuals  # noqa: F401
from . import isolation  # noqa: F401
from . import note_intake  # noqa: F401

__all__ = ["load_library", "library_path", "OwError", "WurliEngine", "EnginePool", "VoiceState", "render_note", "batch_render", "normalize_scale", "tremolo_prefetch", "tremolo_configure", "tremolo_export", "tremolo_import", "features", "alias_audit", "midi_render", "calibrate", "preamp_bench", "render_poly", "centroid_track", "intermod_audit", "overshoot", "pump", "pump_fit", "pickup_law", "bark_audit", "mlp", "MlpWeights", "mlp_train", "harmonics", "residuals", "isolation", "note_intake"]
