"""scrubvae.get.data counterpart (reference: src/scrubvae/get/data.py:46-146, the "full" branch after the h5 read): a loader
whose batches are built on the device from the resident recording instead of a DataLoader over preprocessed windows."""
from __future__ import annotations

import torch

AVG_SPEED_3D_NORM = {"mean": (0.4993, 0.7112, 0.6663), "std": (0.4038, 0.3586, 0.4169)}  # get/data.py:58-63


def device_data(data_config, pose, ids, skeleton_config, train_val_test="train", data_keys=["x6d", "root", "offsets"], shuffle=False,
                stride=2, window=51, speed_threshold=2.25, device="cuda", seed=0, rank=0, world=1):
    """`mouse_data` on a recording already read: pose [frames, J, 3], ids [frames] -> DeviceWindowLoader.

    batch_size, direction_process, arena_size and dataset come from `data_config`.  avg_speed_3d is normalised with the
    reference's constants (kept as `dataset.norm_params`); `discrete_classes["ids"]` is the sorted unique ids; for dataset
    "parkinsons" ids >= 36 are shifted down by 36 and `pd_label` ([n, 1] long, 1 for those ids) is served when asked for.
    `fluorescence` needs the dataset's metadata csv and is not provided."""
    from ..data.recording import DeviceRecording, DeviceWindowLoader
    if "fluorescence" in data_keys:
        raise ValueError("device_data does not provide 'fluorescence' (it is read from the dataset's metadata csv)")
    norm_params = {"avg_speed_3d": {k: torch.tensor(v, dtype=torch.float32) for k, v in AVG_SPEED_3D_NORM.items()}}
    keys = list(data_keys) + ([] if "ids" in data_keys else ["ids"])
    dataset = DeviceRecording(pose, ids, skeleton_config, window, stride, keys, speed_threshold, data_config["direction_process"],
                              norm_params=norm_params, arena_size=data_config["arena_size"], label=train_val_test, device=device)
    labels, discrete_classes = dataset.window_labels, {}
    if data_config["dataset"] == "parkinsons":
        sick = labels["ids"] >= 36
        if "pd_label" in data_keys:
            labels["pd_label"] = sick.long()[:, None]
            discrete_classes["pd_label"] = torch.unique(labels["pd_label"], sorted=True).cpu()
        labels["ids"] = torch.where(sick, labels["ids"] - 36, labels["ids"])
        discrete_classes["ids"] = torch.arange(len(torch.unique(labels["ids"]))).long()
    else:
        discrete_classes["ids"] = torch.unique(labels["ids"], sorted=True).cpu()
    dataset.discrete_classes = discrete_classes
    return DeviceWindowLoader(dataset, data_config["batch_size"], shuffle, seed, rank, world)
