"""What the multi-process tests share (test_dist_cpu.py, test_dist_gpu.py, test_gpu_bench_ranks.py)."""
import socket


def free_port():
    """A TCP port nobody listens on, for a process group's rendezvous on this host."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port
