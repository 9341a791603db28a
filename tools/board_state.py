"""The board a measurement ran on, as a dict for the measurement's JSON: device name and count, torch / HIP versions, and -- read
only -- the clocks, power and utilisation rocm-smi reports at that moment (another tenant's work on the same board shows there).

    python tools/board_state.py            (prints the snapshot)"""
import json
import subprocess
import time


def snapshot():
    import torch
    s = {"time": time.strftime("%Y-%m-%dT%H:%M:%S"), "torch": torch.__version__, "hip": getattr(torch.version, "hip", None)}
    if torch.cuda.is_available():
        p = torch.cuda.get_device_properties(0)
        s.update(device=p.name, arch=getattr(p, "gcnArchName", None), compute_units=p.multi_processor_count,
                 memory_GiB=round(p.total_memory / 2 ** 30, 1), visible_devices=torch.cuda.device_count())
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--showuse", "--json"], capture_output=True, text=True, timeout=20).stdout
        smi = json.loads(out)
        s["rocm_smi_card0"] = smi.get("card0", smi)
    except Exception as e:          # noqa: BLE001  (no rocm-smi, or no permission: say so in the record)
        s["rocm_smi_card0"] = "unavailable: %s" % type(e).__name__
    return s


if __name__ == "__main__":
    print(json.dumps(snapshot(), indent=1))
