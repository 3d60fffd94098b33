"""Loader for the committed golden transition vectors (tests/golden/*.npz)."""
import glob
import os

import numpy as np

from sequential_social_dilemma_games_amd import constants as K

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def default_lut():
    lut = np.zeros((128, 3), dtype=np.uint8)
    for table in (K.DEFAULT_COLOURS, K.CLEANUP_COLOURS):
        for ch, rgb in table.items():
            lut[ord(ch)] = rgb
    return lut


class Group(object):
    def __init__(self, path):
        self.name = os.path.basename(path)[:-4]
        z = np.load(path)
        self.game = int(z["game"])
        self.map = [str(r) for r in z["map"]]
        self.N = int(z["N"])
        self.view_len = int(z["view_len"])
        self.seed = int(z["seed"])
        self.env = int(z["env"])
        self.steps = {k[2:]: z[k] for k in z.files if k.startswith("s_")}
        self.resets = {k[2:]: z[k] for k in z.files if k.startswith("r_")}
        self.n_steps = len(self.steps["t"]) if self.steps else 0
        self.n_resets = len(self.resets["episode"]) if self.resets else 0
        # spawn-table fixtures (t??_*.npz): the probabilities the reference's constants were rebound to and their thresholds
        self.tables = {k[4:]: z[k] for k in z.files if k.startswith("tab_")}

    @property
    def harvest_thresholds(self):
        """uint64 [4] or None (the reference's constants)."""
        return self.tables.get("harvest")

    @property
    def cleanup_thresholds(self):
        """(apple, waste) uint64 [potential_waste_area + 1] each, or None."""
        return (self.tables["cleanup_apple"], self.tables["cleanup_waste"]) if "cleanup_apple" in self.tables else None


def groups():
    return [Group(p) for p in sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))]


def group_names():
    return [os.path.basename(p)[:-4] for p in sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))]


def load(name):
    return Group(os.path.join(GOLDEN_DIR, name + ".npz"))
