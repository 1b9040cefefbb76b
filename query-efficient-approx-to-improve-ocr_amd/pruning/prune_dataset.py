"""`python pruning/prune_dataset.py --dataset pos --cers_tess_path strips.json --prune_method FL --prune_prop 10` — drop-in for the
reference's pruning/prune_dataset.py (:1-121): strip CERs -> mean CER per document -> the kept documents, written as
`cers_<dataset>.json` and `cers_<dataset>_<method>_<prop>.json` under properties.cer_artifacts_path (relative to the working
directory, as in the reference: run from pruning/, the trainers read `pruning/cer_artifacts/NAME.json`).

[new] --backend {hip,cpu} places the FL selection, --features history ranks documents by their last --history_len per-epoch mean
CERs (a trainer's all_cers.json) instead of one mean.  wandb and matplotlib are optional: without them nothing is uploaded and no
histogram is drawn."""
import json
import os
import sys
from collections import defaultdict
from pprint import pprint

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

import properties  # noqa: E402
from pruning import methods  # noqa: E402
from qea._lib import QeaError  # noqa: E402
from qea.cli_flags import build_parser as _build_parser  # noqa: E402

prune_method_mapping = {"topk": methods.topk, "FL": methods.facility_location}


def build_parser():
    return _build_parser("r", "Prunes a dataset by the CERs of its text strips")


def save_hist(data, file_name):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return
    plt.hist(list(data), bins=20)
    plt.xlabel("Average CER")
    plt.ylabel("Count")
    plt.title("CER Histogram")
    plt.savefig(f"{file_name}.png")
    plt.close()


def _wandb_run():
    """the active wandb run, or None when wandb is absent, not initialised or disabled"""
    try:
        import wandb
    except ImportError:
        return None
    run = wandb.run
    if run is None or getattr(run, "disabled", False) or "Disabled" in type(getattr(run, "mode", None)).__name__:
        return None
    return run


def document_of(strip_name):
    return strip_name.split("_", 2)[-1]


class DatasetPruner:
    def __init__(self, args):
        print("Dataset Pruning Arguments")
        pprint(vars(args))
        self.cers_tess_path = args.cers_tess_path
        with open(self.cers_tess_path, "r") as f:
            self.cers = json.load(f)
        self.dataset = args.dataset
        self.method_name = args.prune_method
        self.method = prune_method_mapping[self.method_name]
        self.prune_prop = args.prune_prop
        self.backend = getattr(args, "backend", None)
        self.features = getattr(args, "features", "mean") or "mean"
        self.history_len = getattr(args, "history_len", 8)
        if self.features == "history" and self.method_name != "FL":
            raise QeaError("--features history ranks by facility location: pass --prune_method FL")
        if self.features == "history" and not 1 <= self.history_len <= 32:
            raise QeaError(f"--history_len {self.history_len} outside 1..32")
        os.makedirs(properties.cer_artifacts_path, exist_ok=True)  # In case the artifacts folder does not exist

    def get_image_metric(self):
        if self.features == "history":
            return self.get_image_history()
        print("Calculating mean CER for each document images...")
        cer_groups = defaultdict(list)
        for strip_name, cer in self.cers.items():
            cer_groups[document_of(strip_name)].append(cer)
        cer_means = dict()
        for img_name, cers in cer_groups.items():
            cer_means[img_name] = round(sum(cers) / len(cers), 3)
        print("Completed.")
        return cer_means

    def get_image_history(self):
        """[new] name -> [mean CER of the document's strips in each of the last L epochs], L = min(--history_len, shortest history)."""
        print("Calculating per-epoch mean CERs for each document images...")
        bad = [n for n, h in self.cers.items() if not isinstance(h, list) or not h]
        if bad:
            raise QeaError(f"{self.cers_tess_path}: --features history needs a non-empty list of per-epoch CERs per strip "
                           f"(a trainer's all_cers.json); {len(bad)} entries have none, e.g. {bad[0]!r}")
        L = min(self.history_len, min(len(h) for h in self.cers.values()))
        groups = defaultdict(list)
        for strip_name, hist in self.cers.items():
            groups[document_of(strip_name)].append(hist[-L:])
        out = {name: [round(sum(h[e] for h in hs) / len(hs), 3) for e in range(L)] for name, hs in groups.items()}
        print("Completed.")
        return out

    def prune(self, cer_means):
        print(f"Pruning {self.prune_prop}% of {self.dataset} dataset using {self.method_name} method.")
        num_samples = len(cer_means) - int(len(cer_means) * (self.prune_prop / 100))
        if self.method_name == "FL":
            pruned_data = self.method(cer_means, num_samples, backend=self.backend)
        else:
            pruned_data = self.method(cer_means, num_samples)
        print(f"Size before pruning: {len(cer_means)}, Size after pruning: {len(pruned_data)}")
        return pruned_data

    def save_artifact(self, cer_means, file_name):
        file_path = os.path.join(properties.cer_artifacts_path, f"{file_name}.json")
        with open(file_path, "w") as f:
            json.dump(dict(cer_means), f)
        print(f"Saved dataset information at {file_path}")
        run = _wandb_run()
        if run is not None:
            import wandb
            artifact = wandb.Artifact(type="subset_info", name=file_name)
            artifact.add_file(file_path)
            run.log_artifact(artifact)
        return file_path


def main(argv=None):
    args = build_parser().parse_args(argv)
    pruner = DatasetPruner(args)
    cer_means = pruner.get_image_metric()
    cer_file_name = f"cers_{args.dataset}"
    pruner.save_artifact(cer_means, cer_file_name)

    pruned = pruner.prune(cer_means)
    pruned_file_name = f"{cer_file_name}_{args.prune_method}_{args.prune_prop}"
    pruner.save_artifact(pruned, pruned_file_name)

    # Visualize histogram after pruning (mean-CER features only: a history has no single value per document)
    if pruner.features == "mean":
        save_hist(pruned.values(), "new_topk")
    return pruned


if __name__ == "__main__":
    main()
