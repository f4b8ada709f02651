// Host check of the library's error channel (ace_amd/csrc/errors.h, errors.cpp - the very file the library links): fail returns its
// code, last_error returns the message and its pointer stays put until the thread's next fail, every getter of the C ABI reads the
// same string, and two threads failing at the same time each read their own message.
//   g++ -O2 -std=c++17 -pthread tests/emul/errors_emul.cpp ace_amd/csrc/errors.cpp -o errors_emul && ./errors_emul
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "../../ace_amd/csrc/errors.h"
#include "../../include/ace_sfno.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);    \
            ++failures;                                               \
        }                                                             \
    } while (0)

static int passes_code_on() {
    ACE_TRY(ace::fail(ACE_ERR_STATE, "from ACE_TRY"));
    return ACE_OK;
}

int main() {
    EXPECT(ace::fail(ACE_ERR_INVALID, "first") == ACE_ERR_INVALID);
    EXPECT(std::strcmp(ace::last_error(), "first") == 0);
    EXPECT(ace::fail(ACE_ERR_RUNTIME, std::string("second: ") + "why") == ACE_ERR_RUNTIME);
    const char* p = ace::last_error();
    EXPECT(std::strcmp(p, "second: why") == 0);
    // reading changes nothing: the same pointer and bytes until the next fail of this thread
    const char* (*getters[])(void) = {ace_last_error, ace_mask_last_error, ace_couple_last_error, ace_diag_last_error,
                                      ace_physics_last_error, ace_hpx_last_error, ace_ll_last_error, ace_ocean_phys_last_error,
                                      ace_ocean_derive_last_error, ace_ice_budget_last_error, ace_pixel_mlp_last_error,
                                      ace_disco_last_error};
    for (auto g : getters) EXPECT(g() == p && std::strcmp(g(), "second: why") == 0);
    EXPECT(ace::last_error() == p);
    EXPECT(passes_code_on() == ACE_ERR_STATE && std::strcmp(ace::last_error(), "from ACE_TRY") == 0);

    // two threads fail over and over at the same time: each reads its own message, the main thread's is untouched
    ace::fail(ACE_ERR_INVALID, "main");
    std::atomic<int> ready{0}, bad{0};
    auto work = [&](int id) {
        ++ready;
        while (ready.load() < 2) std::this_thread::yield();
        for (int i = 0; i < 20000; ++i) {
            const std::string m = "thread " + std::to_string(id) + " failure " + std::to_string(i) + std::string(i % 97, 'x');
            if (ace::fail(-10 - id, m) != -10 - id) ++bad;
            const char* q = ace::last_error();
            if (m != q || q != ace_diag_last_error() || q != ace::last_error()) ++bad;
        }
    };
    std::thread a(work, 1), b(work, 2);
    a.join();
    b.join();
    EXPECT(bad.load() == 0);
    EXPECT(std::strcmp(ace::last_error(), "main") == 0);

    if (failures) return 1;
    std::printf("error channel ok\n");
    return 0;
}
