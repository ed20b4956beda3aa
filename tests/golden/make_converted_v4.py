"""Fixture made by the REFERENCE's own converter: tests/golden/converted_v4.st.

    python tests/golden/make_converted_v4.py       (needs the reference checkout; run from the repo root)

A tiny RWKV-4 checkpoint in BlinkDL's layout (for V4 the converter renames and transposes nothing: it only casts to fp16 and lower-cases
the keys, convert_safetensors.py:36-47, 62-72) is saved with torch.save and run through the reference converter exactly as
`make_converted.py` does for V5 / V6 / V7 (`run_reference_converter.py`).  Only the converter's output bytes are committed; `source()`
rebuilds the original tensors from the seed."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_converted as MC  # noqa: E402
from tests import v4_ref  # noqa: E402

CASE = (4, 2, 128, 128, 64, 64)          # version, L, C, F, V, seed
FIXTURE = os.path.join(HERE, "converted_v4.st")


def source() -> dict:
    """the original-layout tensors (numpy fp16), deterministic"""
    _, L, C, F, V, seed = CASE
    return v4_ref.synth_checkpoint_v4(L, C, F, V, seed=seed)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        data = MC.run_converter(source(), d)
    with open(FIXTURE, "wb") as f:
        f.write(data)
    print(f"converted_v4.st: {len(data)} bytes")
