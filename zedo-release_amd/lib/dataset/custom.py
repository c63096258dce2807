"""In-the-wild dataset container (reference lib/dataset/custom.py, a template that does not run as shipped:
undefined names at :31,:47,:60 - SURVEY.md 2, row 9).  This version is the working minimum for
run/inference.py: 2D detections + intrinsics, optional 3D labels for `--eval`.

    CustomDataset(db_2d [N,17,3]=(u,v,conf), camera_param [N,3,3], db_3d=None [N,17,3] metres, seq_start=None)
    CustomDataset.from_npz(path)   # arrays `db_2d`, `camera_param`, optional `db_3d`, optional `seq_start`

seq_start [n_seq+1]: the frames of a video come as clips - clip s is the frames seq_start[s] .. seq_start[s+1]-1 (strictly ascending
from 0 to N; default: one clip, [0, N]).  Read by run.inference --select temporal, which never links the last frame of one clip to the
first frame of the next.
"""
import numpy as np

from ._eval import hypothesis_min


def validate_seq_start(seq_start, N):
    """-> int32 [n_seq+1], strictly ascending from 0 to N (None: one clip, [0, N]); anything else is a ValueError.  Checked here, on
    the host: the device code that walks the clips only clamps."""
    if seq_start is None:
        return np.array([0, N], np.int32)
    a = np.asarray(seq_start)
    if a.ndim != 1 or a.size < 2 or not (np.issubdtype(a.dtype, np.integer) or (np.issubdtype(a.dtype, np.floating) and (a == np.floor(a)).all())):
        raise ValueError(f"seq_start: a 1-D array of at least two integers expected, got {a!r}")
    a = a.astype(np.int64)
    if a[0] != 0 or a[-1] != N or (np.diff(a) <= 0).any():
        raise ValueError(f"seq_start must be strictly ascending from 0 to the number of frames ({N}), got {a.tolist()}")
    return a.astype(np.int32)


class CustomDataset:
    def __init__(self, db_2d, camera_param, db_3d=None, sample_interval=None, seq_start=None):
        self.db_2d = np.asarray(db_2d, dtype=np.float32)
        self.camera_param = np.asarray(camera_param, dtype=np.float32)
        if self.db_2d.ndim != 3 or self.db_2d.shape[1:] != (17, 3) or self.camera_param.shape[1:] != (3, 3):
            raise ValueError("expected db_2d [N,17,3] = (u, v, confidence) and camera_param [N,3,3]")
        self.has_labels = db_3d is not None
        self.db_3d = (np.zeros_like(self.db_2d) if db_3d is None else np.asarray(db_3d, dtype=np.float32))
        if sample_interval:
            self.db_2d, self.db_3d = self.db_2d[::sample_interval], self.db_3d[::sample_interval]
            self.camera_param = self.camera_param[::sample_interval]
        self.real_data_len = len(self.db_2d)
        if seq_start is not None and sample_interval:
            raise ValueError("seq_start together with sample_interval: the clip offsets count the frames as given, not the sampled ones")
        self.seq_start = validate_seq_start(seq_start, len(self.db_2d))

    @classmethod
    def from_npz(cls, path, sample_interval=None):
        d = np.load(path)
        return cls(d["db_2d"], d["camera_param"], d["db_3d"] if "db_3d" in d.files else None, sample_interval,
                   d["seq_start"] if "seq_start" in d.files else None)

    def __len__(self):
        return len(self.db_2d)

    def gt_centred(self):
        gt = self.db_3d.astype(np.float64)
        return gt - gt[:, 0:1]

    def eval_multi(self, preds, protocol2=False, print_verbose=False, sample_interval=None, valid_ind=None, joint=17, row_offset=0):
        """Best-of-H mean (PA-)MPJPE (reference :62-108)."""
        if not self.has_labels:
            raise RuntimeError("this dataset has no 3D labels: run without --eval")
        print("eval multi-hypothesis...")
        best, idx = hypothesis_min(preds, self.gt_centred(), protocol2, valid_ind, row_offset)
        error = float(np.mean(best))
        print(f"mean PA-MPJPE : {error}" if protocol2 else f"mean MPJPE : {error}")
        self.last_best, self.last_index = best, idx
        return error
