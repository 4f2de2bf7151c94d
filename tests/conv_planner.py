"""descriptor -> what the host planner (vps_amd/csrc/conv_plan.cpp) does with it, for GPU tests that assert the kernel they ran:
the stand-alone planner of tests/test_conv_plan.py (host C++, no GPU), default switches, the limits recorded in
tests/conv_plan_cases.json. Wrapped by the `planned_kernel` fixtures of the test files."""
import json
import subprocess

import test_conv_plan


def make_planner(tmp):
    """compiles the driver into `tmp` -> check(d) = (kernel name, needs_reduce, error code of vpsi_conv_check / vpsi_conv_plan)"""
    table = json.load(open(test_conv_plan.TABLE))
    test_conv_plan._plans(tmp, dict(int_fields=table['int_fields'], limits=table['limits'], rows=[]))      # compiles the driver
    lim = table['limits']

    def check(d):
        words = [lim['cus']] + lim['pw_per_cu'] + lim['thin_per_cu']
        for f in table['int_fields']:
            words.append(getattr(d, f[:-3])[int(f[-2])] if f.endswith(']') else getattr(d, f))
        for f in test_conv_plan.POINTERS:
            v = getattr(d, 'inp' if f == 'in' else f)
            words.append(16 + (v & 15) if v else 0)
        words += [1] * len(test_conv_plan.SWITCHES)
        out = subprocess.run([str(tmp / 'plan_driver')], input=' '.join(str(w) for w in words), capture_output=True, text=True, check=True).stdout.split()
        return out[0], int(out[3]), int(out[4])
    return check


def planned_kernel(tmp):
    """-> plan(d) = name of the kernel vpsi_conv_plan gives the descriptor; the descriptor must pass vpsi_conv_check"""
    check = make_planner(tmp)

    def plan(d):
        name, _, err = check(d)
        assert err == 0, (name, err)
        return name
    return plan
