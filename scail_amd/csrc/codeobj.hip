// Host side of the embedded code objects (the generated kernels of scail_amd/asmgen, common.h): the loader and the device's CU count.
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"

// Code objects and kernel handles belong to ONE device: they are cached per HIP device id, so a process that drives several GPUs (a DiT
// on cuda:0 and another engine on cuda:1, a threaded multi-GPU host) launches the module loaded on the device that is current at the call.
static std::mutex g_mutex;
static std::map<std::pair<int, const void*>, hipModule_t> g_modules;                      // (device, image) -> loaded code object
static std::map<std::tuple<int, const void*, std::string>, hipFunction_t> g_functions;    // (device, image, kernel name)
static std::map<int, int> g_cus;                                                          // device -> compute units

int scail_module_function(const char* family, const void* image, const std::string& name, hipFunction_t* fn) {
    std::lock_guard<std::mutex> lk(g_mutex);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        scail_set_error(std::string(family) + ": hipGetDevice failed");
        return 2;
    }
    auto key = std::make_tuple(dev, image, name);
    auto it = g_functions.find(key);
    if (it == g_functions.end()) {
        auto mit = g_modules.find(std::make_pair(dev, image));
        if (mit == g_modules.end()) {
            hipModule_t mod = nullptr;
            hipError_t e = hipModuleLoadData(&mod, image);
            if (e != hipSuccess) {
                scail_set_error(std::string(family) + ": hipModuleLoadData failed: " + hipGetErrorString(e));
                return 2;
            }
            mit = g_modules.emplace(std::make_pair(dev, image), mod).first;
        }
        hipFunction_t f;
        hipError_t e = hipModuleGetFunction(&f, mit->second, name.c_str());
        if (e != hipSuccess) {
            scail_set_error(std::string(family) + ": kernel " + name + " is not in the embedded code object: " + hipGetErrorString(e));
            return 2;
        }
        it = g_functions.emplace(key, f).first;
    }
    *fn = it->second;
    return 0;
}

int scail_device_cus() {
    std::lock_guard<std::mutex> lk(g_mutex);
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        scail_set_error("scail_device_cus: hipGetDevice failed");
        return 0;
    }
    auto it = g_cus.find(dev);
    if (it != g_cus.end()) return it->second;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
        scail_set_error("scail_device_cus: the device's compute-unit count is not available (hipDeviceAttributeMultiprocessorCount)");
        return 0;
    }
    return g_cus[dev] = n;
}
