"""Balance the ground truth of a segmentation training set by the classes its images hold.

Reads a ``train.json`` as ``create_dataset_for_segmentation.py --ground-truth`` writes it (entries with ``has_<class>`` truth
values), sorts every entry into the group ``all`` (every class present), ``none`` (no class present) or, otherwise, into one
group per class it holds, keeps as many entries of every group as the smallest group has, shuffles what is kept and writes it
next to the input as ``<stem>_balanced.json``.  ``--seed`` makes the choice repeatable.
"""
import argparse
import json
import random
from pathlib import Path


def group_entries(entries):
    """group name -> entries, groups in the order they first appear."""
    keys = [key for key in entries[0] if key.startswith("has_")] if entries else []
    groups = {}
    for entry in entries:
        present = [key for key in keys if entry.get(key)]
        if keys and len(present) == len(keys):
            names = ["all"]
        elif not present:
            names = ["none"]
        else:
            names = present
        for name in names:
            groups.setdefault(name, []).append(entry)
    return groups


def balance(entries, rng=random):
    groups = group_entries(entries)
    if not groups:
        return [], 0
    keep = min(len(members) for members in groups.values())
    kept = []
    for members in groups.values():
        members = list(members)
        rng.shuffle(members)
        kept.extend(members[:keep])
    rng.shuffle(kept)
    return kept, keep


def main(argv=None):
    parser = argparse.ArgumentParser(description="Take train gt for semantic segmentation training and balance it")
    parser.add_argument("gt", help="Path to JSON holding gt to balance")
    parser.add_argument("--seed", type=int, default=None, help="seed of the shuffles (default: not seeded)")
    args = parser.parse_args(argv)
    source = Path(args.gt)
    with source.open() as f:
        entries = json.load(f)
    kept, keep = balance(entries, random.Random(args.seed) if args.seed is not None else random)
    print(f"keeping {keep} files per class")
    destination = source.parent / f"{source.stem}_balanced.json"
    with destination.open('w') as f:
        json.dump(kept, f)
    return destination


if __name__ == "__main__":
    main()
