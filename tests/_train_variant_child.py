"""Helper of tests/test_gpu_train_variants.py::test_environment_switch_paths_in_child_processes: train_wgrad.hip and train_roi.hip read their
environment switches once per process, so each setting runs the fixed subset of cases in a process of its own.  argv: out_prefix repo_root"""
import os
import sys
sys.path.insert(0, sys.argv[2])
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import test_gpu_train_variants as tv
tv.child_main(sys.argv[1])
