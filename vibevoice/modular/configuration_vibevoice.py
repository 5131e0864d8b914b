"""`vibevoice.modular.configuration_vibevoice.VibeVoiceConfig` over VVConfig: what the reference fork's 4-bit branch imports to build the
`config=` it passes to from_pretrained (VibeVoiceConfig.from_pretrained(<local dir>), then from_pretrained(..., config=base_config))."""
import copy
import json
import os

from vibevoice_rocm_amd.config import VVConfig


class VibeVoiceConfig(VVConfig):
    """A VVConfig that remembers the config.json it was read from: to_dict() gives that object back (or, for a config built from numbers,
    the reference's schema for its shapes)."""

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **ignored) -> "VibeVoiceConfig":
        """Local directories only (subfolder= joins the path); the hub arguments (cache_dir, local_files_only, ...) are ignored."""
        path = str(pretrained_model_name_or_path)
        if ignored.get("subfolder"):
            path = os.path.join(path, ignored["subfolder"])
        with open(os.path.join(path, "config.json")) as f:
            return cls.from_dict(json.load(f))

    @classmethod
    def from_dict(cls, j: dict, **ignored) -> "VibeVoiceConfig":
        c = cls(**VVConfig.from_json_dict(j).as_dict())
        c._json = copy.deepcopy(j)
        return c

    def to_dict(self) -> dict:
        j = getattr(self, "_json", None)
        if j is not None:
            return copy.deepcopy(j)
        j = self.to_reference_json()
        j["tie_word_embeddings"] = bool(self.tie)
        return j
