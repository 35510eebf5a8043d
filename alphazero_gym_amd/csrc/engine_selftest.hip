// engine_selftest.hip -- the C ABI's diagnostics: the math / MFMA / latency probes (azg_math_selftest) and the stamp buffer of the
// -DAZG_STAMPS builds (azg_debug_stamps).
#include "engine_host.h"
#include "probe_kernels.cuh"

extern "C" {

// diagnostic (-DAZG_STAMPS builds): per-wave cycle sums [n_workgroups*4][16]; returns the number of rows
int azg_debug_stamps(azg_engine* e, unsigned long long* out, size_t max_rows) {
    if (!e || !out) return AZG_E_INVALID;
    size_t rows = e->stamp_n;
    if (rows > max_rows) rows = max_rows;
    ON_DEVICE(e);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(out, e->P.stamps, rows * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (int)rows;
}

int azg_math_selftest(int device_id, int fn_id, const double* in, double* out, size_t n) {
    if (!in || !out || n == 0) return AZG_E_INVALID;
    DeviceScope scope(device_id);
    if (!scope.ok) return AZG_E_DEVICE;
    DeviceAllocs mem;   // (freed before `scope` restores the caller's device)
    double* const di = mem.alloc<double>(n);
    double* const dout = mem.alloc<double>(n);
    if (!di || !dout) return AZG_E_DEVICE;
    int rc = AZG_OK;
    if (hipMemcpy(di, in, n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = AZG_E_DEVICE;
    if (rc == AZG_OK) {
        if (fn_id == 100) {
            int K = (int)((n - 1) / 2);
            hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, di, dout, K);
        } else if (fn_id == 102 && n >= 16) {
            // out[0..11] = shader cycles per dependent operation (see latency_probe_kernel)
            std::vector<int> hc(1 << 16);
            for (size_t i = 0; i < hc.size(); ++i) hc[i] = (int)((i * 4099 + 77) & (hc.size() - 1));
            if (int* chase = mem.alloc<int>(hc.size())) {
                (void)hipMemcpy(chase, hc.data(), hc.size() * 4, hipMemcpyHostToDevice);
                hipLaunchKernelGGL(latency_probe_kernel, dim3(1), dim3(64), 0, 0, dout, chase, 4096);
                (void)hipDeviceSynchronize();
            }
        } else if (fn_id == 101 && n >= 8) {
            // in = [workgroups, iterations, launches]; out = [cycles, 100 MHz ticks, -, ms per launch, TFLOP/s]
            const int wgs = (int)in[0], iters = (int)in[1], reps = (int)in[2] > 0 ? (int)in[2] : 1;
            hipEvent_t e0, e1;
            (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
            hipLaunchKernelGGL(mfma_rate_kernel, dim3(wgs), dim3(256), 0, 0, dout, iters);
            (void)hipEventRecord(e0, 0);
            for (int r = 0; r < reps; ++r) hipLaunchKernelGGL(mfma_rate_kernel, dim3(wgs), dim3(256), 0, 0, dout, iters);
            (void)hipEventRecord(e1, 0);
            (void)hipEventSynchronize(e1);
            float ms = 0.0f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            double res[2] = {ms / reps, (double)wgs * 4 * iters * 16 * 2048.0 / (ms / reps * 1e-3) / 1e12};
            (void)hipMemcpy(dout + 3, res, sizeof(res), hipMemcpyHostToDevice);
            (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        } else {
            hipLaunchKernelGGL(math_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, fn_id, di, dout, n);
        }
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = AZG_E_DEVICE;
    }
    if (rc == AZG_OK && hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = AZG_E_DEVICE;
    return rc;
}

}  // extern "C"
