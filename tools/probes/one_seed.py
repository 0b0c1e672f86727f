"""scratch: one seed of a fuzz body (check_random_configuration / check_random_gather_and_tail), printing the assertion text"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests"))
import parity_cases as T
name, seed = sys.argv[1], int(sys.argv[2])
try:
    getattr(T, name)(seed)
    print(name, seed, "ok")
except AssertionError as e:
    print(name, seed, "FAIL", e)
