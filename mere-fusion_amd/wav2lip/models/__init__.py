from .generator import Wav2Lip  # noqa: F401  (same import path as wav2lip/models/__init__.py:1)
from .syncnet import SyncNet_color  # noqa: F401  (inference-only; the drop-in does not export it: wav2lip.models.syncnet there stays the reference's trainable module)
